"""The torch-free C++ hosts without a device: tests/c_hosts.py's numpy restatement of tests/c_abi_host.h's hash, weight fill
and tensor table holds the header's bits; every host compiles against the present headers and checks its arguments before it
touches the runtime; the parsers of what the hosts print."""
import numpy as np
import pytest

import c_hosts
from oracle import plnerf_oracle as orc

SEQUENCES, INDICES = (0, 23, 100, 123, 997, 998, 999), (0, 1, 2, 65535, 65536, 81663)      # 81,663: the last of 256 x 319
WIDTHS = ((63, 27), (57, 3))

_CPP = r"""
#include "c_abi_host.h"
using namespace c_abi_host;
int main() {      /* no HIP call: the runtime is linked, never initialised */
    const uint32_t ks[] = {%s}, is[] = {%s};
    for (uint32_t k : ks)
        for (uint32_t i : is) { const float h = hashed(k, i); uint32_t b; std::memcpy(&b, &h, 4); std::printf("hashed %%u %%u %%08x\n", k, i, b); }
    const int widths[2][2] = {{63, 27}, {57, 3}};
    for (const auto& w : widths) {
        std::printf("tensors %%d %%d", w[0], w[1]);
        for (const Tensor& t : param_tensors(w[0], w[1])) std::printf(" %%zu:%%d", t.n, t.fan_in);
        std::printf("\n");
        for (int which = 0; which < 2; ++which) {
            const std::vector<float> v = hashed_net_values(which, w[0], w[1]);
            std::printf("net %%d %%d %%d %%zu %%016llx\n", which, w[0], w[1], v.size(), fnv1a(v.data(), v.size() * 4));
        }
    }
    return 0;
}
""" % (", ".join(f"{k}u" for k in SEQUENCES), ", ".join(f"{i}u" for i in INDICES))


def _shapes(widths):
    return {(63, 27): orc.param_shapes, (57, 3): orc.param_shapes_depth}[widths]()


def test_the_numpy_restatement_has_the_headers_bits(tmp_path):
    src = tmp_path / "restated.cpp"
    src.write_text(_CPP)
    run = c_hosts.run(c_hosts.build("restated", tmp_path, source=src))
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = [l.split() for l in run.stdout.split("\n") if l.strip()]
    # the hash
    got = {(int(l[1]), int(l[2])): int(l[3], 16) for l in lines if l[0] == "hashed"}
    assert set(got) == {(k, i) for k in SEQUENCES for i in INDICES}
    for k in SEQUENCES:
        mine = c_hosts.hashed(k, max(INDICES) + 1).view(np.uint32)
        for i in INDICES:
            assert int(mine[i]) == got[(k, i)], (k, i)
    # the tensor table: element counts and fan-ins, in state_dict order
    tables = {(int(l[1]), int(l[2])): [tuple(int(x) for x in t.split(":")) for t in l[3:]] for l in lines if l[0] == "tensors"}
    assert set(tables) == set(WIDTHS)
    for widths in WIDTHS:
        shapes = _shapes(widths)
        by_name = dict(shapes)
        want = [(int(np.prod(shape)), by_name[name.replace("bias", "weight")][1]) for name, shape in shapes]
        assert len(want) == 24 and tables[widths] == want, widths
    # the weight fill: the flat vector is the state_dict's tensors back to back
    nets = {(int(l[1]), (int(l[2]), int(l[3]))): (int(l[4]), int(l[5], 16)) for l in lines if l[0] == "net"}
    assert set(nets) == {(which, widths) for which in (0, 1) for widths in WIDTHS}
    for (which, widths), (count, digest) in nets.items():
        sd = c_hosts.hashed_state_dict(which, _shapes(widths))
        flat = np.concatenate([t.numpy().reshape(-1) for t in sd.values()])
        assert flat.dtype == np.float32 and flat.size == count
        assert c_hosts.fnv1a(flat.tobytes()) == digest, (which, widths)


@pytest.mark.parametrize("name", c_hosts.HOSTS)
def test_every_host_compiles_and_checks_its_arguments_first(name, tmp_path):
    """Run with no arguments, a host prints its usage line and leaves with status 2 -- on a machine without a device, so
    before any call into the runtime or the library."""
    run = c_hosts.run(c_hosts.build(name, tmp_path))
    assert run.returncode == 2 and run.stdout == "", (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert run.stderr.startswith("usage: ") and run.stderr.count("\n") == 1, run.stderr[-2000:]


def test_the_parsers():
    out = "step 0 loss 3e99a3f0 psnr 41200000\nstep 1 loss 3e000000 carve 00000000\nparams 12 18446744073709551615\nss 7 9\n"
    assert c_hosts.parse_steps(out) == [(0x3e99a3f0, 0x41200000), (0x3e000000, 0)]
    assert c_hosts.parse_sums(out, "params") == [12, 2 ** 64 - 1] and c_hosts.parse_sums(out, "ss") == [7, 9]
    assert c_hosts.parse_steps("params 1 2\n") == []
    with pytest.raises(ValueError):
        c_hosts.parse_sums("step 0 loss 00000000 psnr 00000000\nparameters 1 2\n", "params")      # (a prefix is no match)
    with pytest.raises(ValueError):
        c_hosts.parse_sums("", "ss")
    assert c_hosts.parse_planes("rgb8 00000000000000ff\n\ndepth16 cbf29ce484222325\n") == {"rgb8": 0xff, "depth16": 0xcbf29ce484222325}
    assert c_hosts.parse_planes("") == {}
    # FNV-1a 64: the offset basis for no bytes, and the published value for "a"
    assert c_hosts.fnv1a(b"") == 0xcbf29ce484222325 and c_hosts.fnv1a(b"a") == 0xaf63dc4c8601ec8c
