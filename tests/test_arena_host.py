"""The sentinel arena's own tests, on the CPU: the evidence that the detector of tests/test_gpu_containment.py fails when it
should.  (The arena is device-agnostic; the GPU file repeats the planted overrun once on the device.)"""
import pytest
import torch

from arena import Arena, FILL, MIN_GUARD


def _arena():
    a = Arena("cpu", 1 << 20)
    first = a.carve("first", 1000, align=256, role="out")
    ragged = a.carve("ragged", 37 * 4, align=4, role="in")
    ws = a.carve("ws", 4096, align=8, role="zeroed")
    wide = a.carve("wide", 3, align=1, guard_after=200_000, role="scratch")
    return a, first, ragged, ws, wide


def test_carves_are_exact_and_aligned():
    a, first, ragged, ws, wide = _arena()
    assert first.dptr % 256 == 0 and first.u8().numel() == 1000 and first.u8().data_ptr() == first.dptr
    assert ragged.dptr % 4 == 0 and ragged.dptr % 8 != 0, "a 4-byte carve keeps the raggedest start the header allows"
    assert ragged.f32().numel() == 37 and ragged.i32().numel() == 37
    assert ws.dptr % 8 == 0 and ws.dptr % 16 != 0 and ws.f64().numel() == 512
    assert wide.u8().numel() == 3 and wide.guard_after == 200_000
    # the trailing guard begins at the first byte after nbytes; buffers do not overlap and none ends the allocation
    spans = sorted((b.start - b.guard_before, b.start, b.start + b.nbytes, b.start + b.nbytes + b.guard_after)
                   for b in a.buffers.values())
    for (g0, s, e, g1), nxt in zip(spans, spans[1:] + [(a.mem.numel(),) * 4]):
        assert g0 < s <= e < g1 <= nxt[0]
        assert g1 - e >= MIN_GUARD and s - g0 >= 4096
    assert bool((first.u8() == FILL).all()) and bool((ws.u8() == 0).all())
    a.check()


def test_an_arena_that_is_too_small_refuses_the_carve():
    a = Arena("cpu", 4096 + 256 + 100 + MIN_GUARD - 1)
    with pytest.raises(AssertionError, match="too small"):
        a.carve("x", 100 + 256)


def test_a_byte_just_past_a_buffer_is_reported():
    a, first, ragged, ws, wide = _arena()
    a.mem[ragged.start + ragged.nbytes] = 0
    problems = a.problems()
    assert len(problems) == 1 and "`ragged`" in problems[0] and "1 guard byte(s) changed after" in problems[0]
    assert "first 0 and last 0 bytes past its end" in problems[0]
    with pytest.raises(AssertionError, match="`ragged`"):
        a.check()


def test_a_span_far_past_a_buffer_is_reported_with_its_extent():
    a, first, ragged, ws, wide = _arena()
    a.mem[wide.start + wide.nbytes + 150_000:wide.start + wide.nbytes + 150_016] = 7
    problems = a.problems()
    assert len(problems) == 1 and "`wide`" in problems[0] and "16 guard byte(s)" in problems[0]
    assert "first 150000 and last 150015 bytes past its end" in problems[0]


def test_a_byte_just_before_a_buffer_is_reported():
    a, first, ragged, ws, wide = _arena()
    a.mem[ws.start - 1] = 0
    problems = a.problems()
    assert len(problems) == 1 and "`ws`" in problems[0] and "changed before" in problems[0]
    assert "first 1 and last 1 bytes before its start" in problems[0]


def test_a_modified_input_is_reported():
    a, first, ragged, ws, wide = _arena()
    ragged.put(torch.arange(37, dtype=torch.float32))
    ragged.freeze()
    a.check()
    ragged.f32()[5] = -1.0
    problems = a.problems()
    assert len(problems) == 1 and "`ragged`" in problems[0] and "input modified" in problems[0]
    assert "first at offset 22, last at offset 23" in problems[0]      # (5.0 -> -1.0 changes the two high bytes of word 5)


def test_a_zeroed_buffer_left_non_zero_is_reported():
    a, first, ragged, ws, wide = _arena()
    a.check()
    ws.f64()[3] = 1.0
    problems = a.problems()
    assert len(problems) == 1 and "`ws`" in problems[0] and "left non-zero" in problems[0]


def test_a_write_behind_the_last_guard_is_reported():
    a, *_ = _arena()
    a.mem[-1] = 0
    assert any("arena tail" in p for p in a.problems())
