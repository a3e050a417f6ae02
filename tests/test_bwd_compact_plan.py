"""The live-row helpers of pl-nerf_amd/csrc/mlp_bwd_plan.h ("live rows": the 16-bit backward runs over the rows whose
upstream gradient is not exactly zero), checked without a GPU: tests/bwd_compact_plan_dump.cpp is a stand-alone host
program over the header, built the way test_mlp_bwd_plan.py builds its dump.

  * the device-side row ranges bwdplan::live_ranges(n_live, launched) -- the text every weight-gradient workgroup and the
    reduction evaluate, `launched` being the ranges the host's row_ranges(n_rows, cap) put into the grid -- over n_rows in
    test_mlp_bwd_plan.py's ROWS (and the benchmark's 262,144 / 786,432 and the largest count the list holds) x n_live in
    0..n_rows (all of them up to 4,096, then the stage / tile / block edges) x every cap of the three rounds: [0, n_live)
    is covered exactly once, by whole 64-row stages, every range non-empty, never more ranges than the cap, the round or
    the grid the host sized from n_rows (the dealt cap instead of `launched` fails that: 262,144 rows at cap 73 launch 72
    ranges, 73,729 live rows would take 73); n_live = 0 has no range;
  * the head launch over the live rows covers them with no more workgroups than the host launched;
  * the list's chunks and the scan's words lie inside the workspace's partials section, in slots no main launch writes
    ([MAIN_ROUND, MAX_SPLITS)), below PART_PE0 (the first float a thin launch writes in any slot), and no two of them
    share a word.  Each network of a merged call has a workspace of its own, so a list inside its own section cannot
    meet the other network's;
  * the same under every PLNERF_WG_SPLITS worth a build (1, 64, 127; 128 leaves no slot and compiles the feature out);
  * the program once more under -fsanitize=address,undefined (host code only).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pl-nerf_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "bwd_compact_plan_dump.cpp")


def build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bwd_compact_plan")


@pytest.fixture(scope="module")
def dump(tmp):
    return build(tmp, "dump")


def ask(exe, queries):
    out = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert len(lines) == len(queries), out
    return [tuple(int(x) for x in line.split()) for line in lines]


def sweep(exe):
    out = subprocess.run([exe, "sweep"], capture_output=True, text=True, check=True).stdout
    got = dict((m.group(1), (int(m.group(2)), int(m.group(3)))) for m in re.finditer(r"^(\w+) checked=(\d+) bad=(\d+)$", out, re.M))
    assert set(got) == {"ranges", "head", "layout"} and "BAD" not in out, out
    return got


def test_invariants_over_the_sweep(dump):
    got = sweep(dump)
    assert all(bad == 0 for _, bad in got.values()), got
    # every n_live of the six small row counts alone, at every cap of the three rounds: more than a million cases
    assert got["ranges"][0] > 1000000 and got["head"][0] > 10000 and got["layout"][0] == 12, got


def test_literal_answers(dump):
    const = subprocess.run([dump], input="const\n", capture_output=True, text=True, check=True).stdout
    assert const == "slot0=32 slots=96 chunk=524288 block_rows=1024 max_blocks=32752\n"
    # no live row: no range (and no division by zero); then the rule of row_ranges on n_live
    assert ask(dump, ["live_ranges 0 32", "live_ranges 1 32", "live_ranges 64 24", "live_ranges 65 24", "live_ranges 270207 24",
                      "live_ranges 4096 8", "live_ranges 4096 32", "live_ranges 270207 95"]) == \
        [(0, 64), (1, 64), (1, 64), (1, 128), (24, 11264), (4, 1024), (4, 1024), (94, 2880)]
    assert ask(dump, ["live_head 0", "live_head 1", "live_head 4096", "live_head 270207"]) == [(1, 0), (1, 32), (16, 256), (512, 544)]
    # slot 32 is the first one no main launch writes; a slot is 596,608 floats, its PART_MAIN area 524,288, PART_VMAIN behind it
    assert ask(dump, ["entry 0", "entry 524287", "entry 524288", "scan 0", "scan 16"]) == \
        [(32 * 596608,), (32 * 596608 + 524287,), (33 * 596608,), (32 * 596608 + 524288,), (32 * 596608 + 524288 + 16,)]
    # 32,752 count words x 1,024 rows bound the list before its 96 chunks do
    assert ask(dump, ["fits 0", "fits 1", "fits 786432", "fits 33538048", "fits 33538049"]) == [(1,), (1,), (1,), (1,), (0,)]


@pytest.mark.parametrize("splits", [1, 64, 127, 128])
def test_every_main_round_the_header_accepts(tmp, splits):
    exe = build(tmp, f"dump_{splits}", f"-DPLNERF_WG_SPLITS={splits}")
    got = sweep(exe)
    assert all(bad == 0 for _, bad in got.values()), got
    (fits,) = ask(exe, ["fits 1000"])
    if splits == 128:      # the main round takes every slot: no room, the backward stays dense
        assert fits == (0,) and got["layout"][0] == 0
    else:
        assert fits == (1,) and got["layout"][0] >= 11 and ask(exe, ["entry 0"]) == [(splits * 596608,)]


def test_under_the_address_and_undefined_behaviour_sanitizers(tmp):
    exe = build(tmp, "dump_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")
    got = sweep(exe)
    assert all(bad == 0 for _, bad in got.values()), got
    assert ask(exe, ["live_ranges 0 32", "entry 524288", "fits 33538049"]) == [(0, 64), (33 * 596608,), (0,)]
