"""pl-nerf_amd/csrc/mlp_bwd_plan.h, checked without a GPU: the header is plain C++, so a stand-alone program
(tests/mlp_bwd_plan_dump.cpp, built like test_mlp_fwd_route.py builds its dump) prints what the backward's host side decides.

  * invariants over a sweep -- every row count 1..3,000,000 at the single-network caps (half planes 32 / 85 / 127, fp32 56),
    every cap 1..127 on a thinner grid, pairs of networks for the deal, the head launch: every launched row range holds
    a row (an empty one would leave stale workspace in the gradients: the round-4 bug), the ranges cover all rows and are
    whole 64- / 16-row stages, two dealt caps are >= 1 each and sum to the round, the head workgroups cover all rows
    within MAX_HEAD_WGS (empty head workgroups are fine: the head kernel writes zeros for them; 131,073 rows has 56);
  * literal tables of row ranges, deals, head launches and dgrad tiles;
  * the workspace layout: sections in order, back to back, 16-byte aligned, and the total size;
  * the launch scale of the half dz planes (mlp_layout.h: dzh_shift, which the four kernel sites call) over fp32's whole
    exponent range, zero, subnormals, infinity and NaNs.

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


def launch_scale_patterns():
    """fp32 bit patterns of max |g_raw| for the launch-scale sweep: every exponent field at mantissa 0, 1 and all-ones (zero,
    the smallest and the largest subnormal, 2^-124 = 0x01800000 with both neighbours, the largest finite value, infinity and
    two NaN patterns are among them), and a third NaN pattern with the quiet bit."""
    bits = [(e << 23) | m for e in range(256) for m in (0, 1, 0x7fffff)]
    for named in (0, 1, 0x007fffff, 0x017fffff, 0x01800000, 0x01800001, 0x7f7fffff, 0x7f800000, 0x7f800001, 0x7fffffff):
        assert named in bits, hex(named)
    return bits + [0x7fc00000]


def test_launch_scale_of_the_half_dz_planes(dump):
    """mlp_layout.h: dzh_shift, the one derivation of the 16-bit backward's launch scale 2^s (include/plnerf_hip.h, "Backward
    of modes 1-4"), against the contract written out in exact integer arithmetic (fractions, no float rounding):
      finite, max |g_raw| >= 2^-124      s = 4 - e, max |g_raw| = m 2^e with 0.5 <= m < 1 (what frexpf / ldexpf gave before the
                                         derivation was written once), so max |g_raw| 2^s lies in [8, 16);
      0 < max |g_raw| < 2^-124           s = 127, the largest finite scale (the scaled maximum stays below 8);
      0, infinity, any NaN               s = 0;
    and 2^s, 2^-s come back as the fp32 bit patterns of exactly those powers: finite and non-zero for every input."""
    import math
    from fractions import Fraction
    bits = launch_scale_patterns()
    answers = ask(dump, [f"shift {b}" for b in bits])

    def value(b):      # a non-negative finite fp32 bit pattern, exactly
        e, m = b >> 23, b & 0x7fffff
        return Fraction(m, 1 << 23) * Fraction(2) ** -126 if e == 0 else (1 + Fraction(m, 1 << 23)) * Fraction(2) ** (e - 127)

    checked = {"in range": 0, "below": 0, "unscaled": 0}
    for b, (s, up, down) in zip(bits, answers):
        e = b >> 23
        if b == 0 or e == 255:
            want, kind = 0, "unscaled"
        else:
            gm = value(b)
            if gm >= Fraction(2) ** -124:
                want, kind = 4 - math.frexp(float(gm))[1], "in range"      # (every fp32 is a double: frexp is exact)
                assert 8 <= gm * Fraction(2) ** s < 16, (hex(b), s)
            else:
                want, kind = 127, "below"
                assert gm * Fraction(2) ** s < 8, (hex(b), s)
        checked[kind] += 1
        assert s == want, (hex(b), s, want)
        assert -127 <= s <= 127, (hex(b), s)
        # 2^s is a normal number; 2^-s too, but for s = 127: the subnormal 2^-127, one mantissa bit
        assert 0 < up < 0x7f800000 and value(up) == Fraction(2) ** s, (hex(b), s, hex(up))
        assert 0 < down < 0x7f800000 and value(down) == Fraction(2) ** -s, (hex(b), s, hex(down))
    # 253 exponent fields from 3 up at three mantissas | fields 0..2 less zero | zero, infinity and three NaN patterns
    assert checked == {"in range": 252 * 3, "below": 3 * 3 - 1, "unscaled": 1 + 3 + 1}, checked
    # the literal corners: 1.0 -> 3; 2^-124 -> 127 and its neighbour below -> 127 as well; the largest finite -> -124
    assert dict(zip(bits, (a[0] for a in answers)))[0x3f800000] == 3
    by_bits = dict(zip(bits, answers))
    assert by_bits[0x01800000] == (127, 0x7f000000, 0x00400000) and by_bits[0x017fffff][0] == 127 and by_bits[0x02000000][0] == 126
    assert by_bits[0x7f7fffff] == (-124, 0x01800000, 0x7d800000)


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
