"""pl-nerf_amd/csrc/mlp_bwd_plan.h, checked without a GPU: the header is plain C++, so a stand-alone program
(tests/mlp_bwd_plan_dump.cpp, built like test_mlp_fwd_route.py builds its dump) prints what the backward's host side decides.

  * invariants over a sweep -- every row count 1..3,000,000 at the single-network caps (half planes 32 / 85 / 127, fp32 56),
    every cap 1..127 on a thinner grid, pairs of networks for the deal, the head launch: every launched row range holds
    a row (an empty one would leave stale workspace in the gradients: the round-4 bug), the ranges cover all rows and are
    whole 64- / 16-row stages, two dealt caps are >= 1 each and sum to the round, the head workgroups cover all rows
    within MAX_HEAD_WGS (empty head workgroups are fine: the head kernel writes zeros for them; 131,073 rows has 56);
  * literal tables of row ranges, deals, head launches and dgrad tiles;
  * the workspace layout: sections in order, back to back, 16-byte aligned, and the total size.

The tables and sizes were NOT taken from the header: they were written down from the arithmetic of plan_job, wgrad_h16_multi's
deal, head_wgs_for and bwd_launch as they stood in the commit before the header existed (f19716f; a line-for-line port
run by hand), the workspace totals from that commit's plnerf_mlp_bwd_workspace_bytes.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-nerf_amd", "csrc")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mlp_bwd_plan") / "mlp_bwd_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "mlp_bwd_plan_dump.cpp"),
                    "-o", exe], check=True)
    return exe


def ask(exe, queries):
    """One child process: a query per line in, the answer's integers per line out."""
    out = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert len(lines) == len(queries), out
    return [tuple(int(x) for x in line.split()) for line in lines]


def test_invariants_over_the_sweep(dump):
    out = subprocess.run([dump, "sweep"], capture_output=True, text=True, check=True).stdout
    const = subprocess.run([dump], input="const\n", capture_output=True, text=True, check=True).stdout
    # the caps the sweep runs at, and the capacities of the workspace sections they must fit
    assert const == "main_round=32 f32_splits=56 thin_rows=3x85 thin_tiled=2x127 max_splits=128 max_head_wgs=512\n"
    # 4 caps x 3,000,000 + 127 caps x the thinner grid | 3 rounds x 16 partners x the grid x both orders | half and fp32
    grid = 5000 + len(range(5000, 3000001, 977)) + 3 * 9
    assert out == (f"ranges checked={4 * 3000000 + 127 * grid} bad=0\n"
                   f"deal checked={3 * 16 * grid * 2} bad=0\n"
                   "head checked=6000000 bad=0\n"), out


# (n_rows, half, cap): (ranges, rows per range)
RANGES = {
    (131072, 1, 85): (82, 1600),      # the round-4 case: 85 ranges of 1,600 would leave 82..84 empty
    (131072, 1, 32): (32, 4096),
    (1, 1, 32): (1, 64),
    (64, 1, 32): (1, 64),
    (65, 1, 32): (1, 128),
    (1025, 1, 32): (2, 576),
    (8000, 1, 127): (8, 1024),
    (1000000, 1, 127): (127, 7936),
    (1000000, 1, 85): (85, 11776),
    (1, 0, 56): (1, 16),
    (15, 0, 56): (1, 16),
    (16, 0, 56): (1, 16),
    (17, 0, 56): (1, 32),
    (1024, 0, 56): (1, 1024),
    (1025, 0, 56): (2, 528),
    (5600, 0, 56): (6, 944),
    (7448, 0, 56): (8, 944),
    (8000, 0, 56): (8, 1008),
    (57344, 0, 56): (56, 1024),
    (57345, 0, 56): (56, 1040),
    (131072, 0, 56): (56, 2352),
    (1000000, 0, 56): (56, 17872),
}
# two networks, half planes: (rows, rows, round): (caps, (ranges, rows per range) of either network)
DEALS = {
    (262144, 786432, 32): ((8, 24), (8, 32768), (24, 32768)),
    (262144, 786432, 85): ((21, 64), (21, 12544), (64, 12288)),
    (262144, 786432, 127): ((32, 95), (32, 8192), (95, 8320)),
    (8000, 296, 32): ((31, 1), (8, 1024), (1, 320)),
    (8000, 296, 85): ((82, 3), (8, 1024), (1, 320)),
    (8000, 296, 127): ((122, 5), (8, 1024), (1, 320)),
    (2400, 720000, 32): ((1, 31), (1, 2432), (31, 23232)),
    (2400, 720000, 85): ((1, 84), (1, 2432), (84, 8576)),
    (2400, 720000, 127): ((1, 126), (1, 2432), (125, 5760)),
    (1, 1, 32): ((16, 16), (1, 64), (1, 64)),
    (1, 1, 85): ((43, 42), (1, 64), (1, 64)),
    (1, 1, 127): ((64, 63), (1, 64), (1, 64)),
}
# (n_rows, half): (head workgroups, rows per head workgroup)
HEADS = {
    (1, 1): (1, 32), (1, 0): (1, 1),
    (255, 1): (1, 256), (255, 0): (1, 255),
    (256, 1): (1, 256), (256, 0): (1, 256),
    (257, 1): (2, 160), (257, 0): (2, 129),
    (8000, 1): (32, 256), (8000, 0): (32, 250),
    (131072, 1): (512, 256), (131072, 0): (512, 256),
    (131073, 1): (512, 288), (131073, 0): (512, 257),      # half planes: workgroups 456..511 hold no row
    (147456, 1): (512, 288), (147456, 0): (512, 288),
    (147457, 1): (512, 320), (147457, 0): (512, 289),
    (1000000, 1): (512, 1984), (1000000, 0): (512, 1954),
}
DGRAD_TILES = {1: 1, 191: 1, 192: 1, 193: 2, 1000: 6}


def test_literal_tables(dump):
    keys = list(RANGES)
    assert dict(zip(keys, ask(dump, ["ranges %d %d %d" % k for k in keys]))) == RANGES
    keys = list(HEADS)
    assert dict(zip(keys, ask(dump, ["head %d %d" % k for k in keys]))) == HEADS
    keys = list(DGRAD_TILES)
    assert dict(zip(keys, [t for (t,) in ask(dump, ["tiles %d" % k for k in keys])])) == DGRAD_TILES
    # a single network takes the whole round
    assert ask(dump, ["deal 32 8000 0", "deal 127 1 0"]) == [(32, 0), (127, 0)]
    for (n0, n1, rnd), (caps, r0, r1) in DEALS.items():
        (got,) = ask(dump, [f"deal {rnd} {n0} {n1}"])
        assert got == caps, (n0, n1, rnd, got)
        assert ask(dump, [f"ranges {n0} 1 {got[0]}", f"ranges {n1} 1 {got[1]}"]) == [r0, r1], (n0, n1, rnd)


ROWS = (0, 1, 191, 192, 193, 961, 1152, 1153, 1000)
# plnerf_mlp_bwd_workspace_bytes before the header existed, at ROWS: the exact-fp32 mode | every 16-bit mode
TOTAL_FP32 = (306921984, 306931728, 308783088, 308792832, 308802576, 316285968, 318147072, 318156816, 316665984)
TOTAL_HALF = (306922000, 307757600, 307760640, 307760656, 308596256, 311950880, 311953936, 312789536, 311951504)
# section sizes in bytes (mlp_layout.h's numbers, spelt out): 128 row ranges of 596,608 floats of split-K partials, 512 head
# workgroups of 648 floats, G (128 x 256) and s (128); a dz row is 2,432 floats (fp32 mode) or 2,176 halves = 4,352 bytes on
# rows padded to the dgrad tile of 192 (16-bit modes, which also keep 16 bytes of scalars behind the planes)
PARTIALS, HEAD_PART, GRED = 128 * 596608 * 4, 512 * 648 * 4, (128 * 256 + 128) * 4


def test_workspace_layout(dump):
    for half, totals in ((0, TOTAL_FP32), (1, TOTAL_HALF)):
        for n, total in zip(ROWS, totals):
            (w,) = ask(dump, [f"ws {n} {half}"])
            dz, gmax, partials, head_part, gred, g_eff, end = w
            assert all(x % 16 == 0 for x in w), (n, half, w)
            # in order and back to back: each section starts where the one before it ends
            assert dz == 0
            assert gmax == (4352 * ((n + 191) // 192 * 192) if half else 2432 * 4 * n)
            assert partials == gmax + (16 if half else 0)
            assert head_part == partials + PARTIALS
            assert gred == head_part + HEAD_PART
            assert g_eff == gred + GRED
            assert end == g_eff + 16 * n
            assert end == total, (n, half, end, total)
