"""pl-nerf_amd/csrc/mlp_fwd_route.h, checked without a GPU: the header is plain C++, so a stand-alone program
(tests/mlp_fwd_route_dump.cpp, built like test_pe_probe_host.py builds its checker) prints every decision it makes.

  * which forward kernel each 16-bit-mode call runs on -- 2 element types x NS 1 / 2 x training x embedded x 3 fwd_kernel
    values = 48 routes -- and which of the 16 (element, NS, SAVE, EMB) instantiations exist, against a literal table;
  * the header's instantiation list and the Makefile's RR_INST name the same eleven variants.

The table was written down from the two predicates (use_rr, use_rr_bf16) and the eleven mlp_rr_k*_*.hip files the library had
before the header existed, not from the header.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-nerf_amd", "csrc")

# element NS training embedded: the instantiation exists; the register-resident kernel runs under AUTO / RR / PP
TABLE = """\
f16 1 0 0 exists=1 auto=1 rr=1 pp=0
f16 1 0 1 exists=0 auto=0 rr=0 pp=0
f16 1 1 0 exists=1 auto=0 rr=1 pp=0
f16 1 1 1 exists=0 auto=0 rr=0 pp=0
f16 2 0 0 exists=1 auto=1 rr=1 pp=0
f16 2 0 1 exists=1 auto=1 rr=1 pp=0
f16 2 1 0 exists=1 auto=1 rr=1 pp=0
f16 2 1 1 exists=1 auto=1 rr=1 pp=0
bf16 1 0 0 exists=1 auto=1 rr=1 pp=0
bf16 1 0 1 exists=0 auto=0 rr=0 pp=0
bf16 1 1 0 exists=0 auto=0 rr=0 pp=0
bf16 1 1 1 exists=0 auto=0 rr=0 pp=0
bf16 2 0 0 exists=1 auto=1 rr=1 pp=0
bf16 2 0 1 exists=1 auto=1 rr=1 pp=0
bf16 2 1 0 exists=1 auto=1 rr=1 pp=0
bf16 2 1 1 exists=1 auto=1 rr=1 pp=0
"""
INSTANCES = sorted(" ".join(line.split()[:4]).replace(" ", "_") for line in TABLE.splitlines() if "exists=1" in line)


def test_routes_and_instantiation_list(tmp_path):
    exe = str(tmp_path / "mlp_fwd_route_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "mlp_fwd_route_dump.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    decisions = "".join(line + "\n" for line in out.splitlines() if not line.startswith("row "))
    assert decisions == TABLE
    rows = [line[4:] for line in out.splitlines() if line.startswith("row ")]
    assert len(INSTANCES) == 11 and sorted(rows) == INSTANCES and len(set(rows)) == 11
    # the Makefile's list: one object per row, compiled from mlp_rr_inst.hip, and all of them linked
    make = open(os.path.join(CSRC, "Makefile")).read()
    stems = re.search(r"^RR_INST\s*=(.*)$", make, re.M).group(1).split()
    assert sorted(stems) == INSTANCES and len(set(stems)) == 11
    assert re.search(r"^RR_INST_OBJS\s*=\s*\$\(RR_INST:%=mlp_rr_i_%\.o\)\s*$", make, re.M)
    assert re.search(r"^OBJS\s*=.*\$\(RR_INST_OBJS\)", make, re.M) and "-Wl,--no-undefined" in make
