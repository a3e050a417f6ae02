"""pl-nerf_amd/csrc/mlp_unique_plan.h, checked without a GPU: the header is plain C++, so a stand-alone program
(tests/fwd_unique_plan_dump.cpp) prints what it decides.

  * the predicate's table -- who plnerf_mlp_fwd_unique serves -- against the rule restated here: the register-resident kernel
    of the split modes (NS 2, fwd_kernel AUTO or RR), no caller-embedded rows, at least 3 rows per ray, the switch on, and for
    a training forward the backward over live rows; and the library's own predicate with both environment switches;
  * the workspace's layout against the sections restated from include/experimental/plnerf_hip_unique.h, and against what the
    library reports (plnerf_mlp_unique_layout / _workspace_bytes: the carver the kernels use);
  * the list rule as a host function against a numpy model over random run patterns -- once more with the program built under
    AddressSanitizer and UndefinedBehaviorSanitizer.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import abi_support as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-nerf_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "fwd_unique_plan_dump.cpp")


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", *flags, "-I", CSRC, SOURCE, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fwd_unique_plan"), "fwd_unique_plan_dump")


def test_the_predicates_table(exe):
    out = subprocess.run([exe, "table"], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    rows = [line for line in out if line[0] in "fb" and line.split()[0] in ("f16", "bf16")]
    assert len(rows) == 2 * 2 * 2 * 2 * 3 * 4 * 2 * 2
    served = 0
    for line in rows:
        elem, ns, training, emb, forced, spr, compact, enabled, got = line.split()
        ns, training, emb, forced, spr, compact, enabled = (int(v) for v in (ns, training, emb, forced, spr, compact, enabled))
        want = (enabled == 1 and ns == 2 and emb == 0 and forced in (0, 1) and spr >= 3 and (training == 0 or compact == 1))
        assert got == f"served={int(want)}", line
        served += int(want)
    assert served == 2 * 2 * 2 * (1 + 2)      # element x {AUTO, RR} x {3, 192} x (training with the compact backward, inference with either)
    assert "ragged served=0" in out and "beyond-the-live-list training=0 inference=1" in out


def test_the_librarys_predicate_reads_both_switches():
    L = abi.built_lib()
    served = L.lib().plnerf_mlp_fwd_unique_served
    f16x3, bf16x3 = L.PRECISION["f16x3"], L.PRECISION["bf16x3"]
    found = {k: os.environ.pop(k, None) for k in ("PLNERF_FWD_UNIQUE", "PLNERF_BWD_COMPACT")}
    try:
        for prec in (f16x3, bf16x3):
            assert served(prec, 0, 0, 192, 786432, 1) == 1 and served(prec, 0, 0, 192, 786432, 0) == 1
            assert served(prec, 0, L.FWD_KERNELS["rr"], 3, 387, 1) == 1
            assert served(prec, 0, L.FWD_KERNELS["pp"], 192, 786432, 1) == 0      # the pipelined kernel
            assert served(prec, 1, 0, 192, 786432, 1) == 0                        # caller-embedded rows
            assert served(prec, 0, 0, 2, 786432, 1) == 0                          # no row can be interior
            assert served(prec, 0, 0, 192, 786433, 1) == 0                        # no whole rays
        for prec in (L.PRECISION["fp32"], L.PRECISION["f16"], L.PRECISION["bf16"], 7, -1):
            assert served(prec, 0, 0, 192, 786432, 1) == 0 and served(prec, 0, 0, 192, 786432, 0) == 0
        assert served(f16x3, 0, 5, 192, 786432, 1) == 0 and served(f16x3, 0, 0, 192, 0, 1) == 0 and served(f16x3, 0, 0, 0, 192, 1) == 0
        os.environ["PLNERF_BWD_COMPACT"] = "0"      # the dense backward reads every row of the planes: training is not served
        assert served(f16x3, 0, 0, 192, 786432, 1) == 0 and served(f16x3, 0, 0, 192, 786432, 0) == 1
        del os.environ["PLNERF_BWD_COMPACT"]
        os.environ["PLNERF_FWD_UNIQUE"] = "0"
        assert served(f16x3, 0, 0, 192, 786432, 1) == 0 and served(f16x3, 0, 0, 192, 786432, 0) == 0
        os.environ["PLNERF_FWD_UNIQUE"] = "1"
        assert served(f16x3, 0, 0, 192, 786432, 1) == 1
    finally:
        for k, v in found.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _expected_layout(n):
    up = lambda v: -(-v // 256) * 256
    P, blocks = up(n), -(-n // 1024)
    off, out = 0, {}
    for name, nbytes in (("words", (16 + blocks) * 4), ("rows_u", 4 * P), ("src", 4 * P), ("pts_u", 12 * P), ("dirs_u", 12 * P),
                         ("raw_u", 16 * P), ("g_raw_u", 16 * P), ("absmax", 4 * blocks)):
        out[name] = off
        off += up(nbytes)
    out["total"], out["n_absmax"] = off, blocks
    return out


def test_the_workspace_against_the_carver(exe):
    L = abi.built_lib()
    sizes = (1, 3, 255, 256, 257, 387, 448, 1024, 1025, 786432, 4 * 1024 * 1024 + 5)
    out = subprocess.run([exe, "layout"] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=60).stdout
    for n, line in zip(sizes, out.splitlines()):
        want = _expected_layout(n)
        fields = dict(kv.split("=") for kv in line.split(": ")[1].split())
        assert int(fields["padded"]) == -(-n // 256) * 256 and int(fields["blocks"]) == want["n_absmax"], (n, line)
        for name in ("words", "rows_u", "src", "pts_u", "dirs_u", "raw_u", "g_raw_u", "absmax", "total"):
            assert int(fields[name]) == want[name], (n, name, line)
        lo = L.UniqueLayout()
        assert L.lib().plnerf_mlp_unique_layout(n, ctypes.byref(lo)) == 0
        assert {name: getattr(lo, name) for name, _ in lo._fields_} == want, n
        assert L.lib().plnerf_mlp_unique_workspace_bytes(n) == want["total"]
    assert L.lib().plnerf_mlp_unique_workspace_bytes(0) == 0 and L.lib().plnerf_mlp_unique_workspace_bytes(-5) == 0
    assert L.lib().plnerf_mlp_unique_layout(0, ctypes.byref(L.UniqueLayout())) == -1
    assert L.lib().plnerf_mlp_unique_layout(387, None) == -1


def model(bits, spr):
    """The rule in numpy on [n, 3] words: (n_eval, rows_u, src)."""
    n = bits.shape[0]
    k = np.arange(n) % spr
    eq = (bits[1:] == bits[:-1]).all(1)
    interior = np.zeros(n, bool)
    interior[1:n - 1] = (k[1:n - 1] != 0) & (k[1:n - 1] != spr - 1) & eq[:-1] & eq[1:]
    ev = ~interior
    return int(ev.sum()), np.nonzero(ev)[0], np.cumsum(ev) - 1


def _cases():
    rng = np.random.default_rng(5)
    for rays, spr in ((1, 1), (1, 3), (5, 2), (129, 3), (60, 7), (9, 192), (33, 24)):
        n = rays * spr
        for mean_run in (1.0, 2.0, 5.0, 200.0):
            # runs of random length over the WHOLE launch, so that runs cross ray boundaries as well
            values = rng.standard_normal((n, 3)).astype(np.float32)
            starts = rng.random(n) < 1.0 / mean_run
            starts[0] = True
            pts = values[np.maximum.accumulate(np.where(starts, np.arange(n), 0))]
            flip = rng.random(n) < 0.1
            pts[flip, 0] = np.where(rng.random(int(flip.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))      # +0 / -0 differ
            yield rays, spr, np.ascontiguousarray(pts).view(np.uint32)


def _check_list(exe, env=None):
    for rays, spr, bits in _cases():
        n = bits.shape[0]
        text = f"{n} {spr}\n" + " ".join(f"{w:x}" for w in bits.reshape(-1)) + "\n"
        out = subprocess.run([exe, "list"], input=text, capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode == 0, (rays, spr, out.returncode, out.stderr[-2000:])
        lines = out.stdout.splitlines()
        n_eval, rows_u, src = model(bits, spr)
        assert int(lines[0]) == n_eval, (rays, spr)
        assert np.array_equal(np.array(lines[1].split(), dtype=np.int64), rows_u), (rays, spr)
        assert np.array_equal(np.array(lines[2].split(), dtype=np.int64), src), (rays, spr)


def test_the_list_rule_on_the_host(exe):
    _check_list(exe)


def test_the_list_rule_under_asan_and_ubsan(tmp_path):
    """The same program, its own main, built with -fsanitize=address,undefined and -fno-sanitize-recover: any report ends the
    run with a non-zero code."""
    san = _build(tmp_path, "fwd_unique_plan_dump_san", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    _check_list(san, env)
    for args in (["table"], ["layout", "1", "387", "786432"]):
        assert subprocess.run([san] + args, capture_output=True, text=True, timeout=60, env=env).returncode == 0
