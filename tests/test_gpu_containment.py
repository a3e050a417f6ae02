"""No entry point writes outside the bytes it is given -- and none depends on what its scratch held, or changes an input.

The C ABI is "caller-owned memory, sizes from the headers".  Every test elsewhere in the suite allocates with torch, whose
allocator rounds up and packs live tensors side by side, so a store past a buffer lands in slack or in a neighbour and
shows up, if ever, as an unrelated wrong number.  Here every buffer of a call is carved at its EXACT size out of one
sentinel arena (tests/arena.py, self-tested in tests/test_arena_host.py) and the call goes through the raw ABI, as a C
caller that packs its buffers tightly would make it.  tests/containment.py describes every entry point once; each case
runs three times on identical inputs -- scratch at 0x00, scratch at 0xFF, and on ordinary torch allocations -- and must
satisfy, exactly (bytes unchanged, bits equal; nothing here has a tolerance):

  (a) after every call, every guard byte of the arena still holds the fill;
  (b) every output is bit-identical between the two fills, and both to the run on ordinary allocations;
  (c) every buffer a call only reads is unchanged by it;
  (d) every "zeroed once, left zeroed" workspace is zero again;
  (e) no 4-byte word of a documented output still holds the fill -- documented padding excepted and named in the table:
      the saved state of the 16-bit modes (rows padded to 256, layout private), the 272 bytes per row of ReLU bit masks
      that plnerf_mlp_saved_bytes counts in fp32 mode too and the fp32 kernels neither write nor read, the columns N..ldc
      of plnerf_gemm_f32's C and a frame's pixels outside a call's range (which must STILL hold the fill), the three
      unused floats behind a one-call gradient block and the three words behind the status word of a packed buffer (not
      touched), outputs the call was given NULL for;
  (f) the return code is PLNERF_OK and every floating-point result is finite.

An overrun lands in memory the test owns: no buffer ends an allocation and no call gets less than its header asks for.

Shapes are the smallest at which a tile edge exists: see the lists at the end of tests/containment.py.  Each entry runs at
the smallest S (or B) of the list its own host check accepts: the prologue entries and the piecewise-linear samplers at
S = 1 (the samplers on hand-made tau, T and weights, since no quadrature can supply them there); the quadrature in both
modes, the linear epilogues and plnerf_sample_const at 2; the constant-mode stages, which need one interior weight, at 3;
the size is in the case id.  The one-call entries run at 67 rays (then 41) of 16 + 16 samples, which every size query
accepts; of their workspace only the loss kernel's block is zeroed in the arena runs, the rest holds the scratch fill.
"""
import pytest
import torch

import containment as C
from arena import Arena
from gpu_support import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from plnerf_amd import _lib
    _lib.lib()
    return _lib


def _params(cases):
    return pytest.mark.parametrize("build", [b for _, b in cases], ids=[i for i, _ in cases])


def test_the_detector_sees_an_overrun_planted_on_the_device():
    """A torch indexing store one float past a carve (and one before another) -- no library call -- is reported with the
    buffer's name and the distance from its end."""
    arena = Arena(dev(), 1 << 20)
    a = arena.carve("a", 37 * 4, align=4, role="out")
    b = arena.carve("b", 512, align=256, role="in")
    b.put(torch.arange(128, dtype=torch.float32, device=dev()))
    b.freeze()
    arena.check()
    arena.mem.view(torch.float32)[(a.start + a.nbytes) // 4 + 2] = 1.0      # words 2 past the end of `a`
    problems = arena.problems()
    assert len(problems) == 1 and "`a`" in problems[0] and "changed after" in problems[0], problems
    assert "4 guard byte(s)" in problems[0] and "first 8 and last 11 bytes past its end" in problems[0], problems
    arena.mem[b.start - 1] = 0
    b.f32()[7] = -7.0
    problems = arena.problems()
    assert len(problems) == 3 and any("`b`" in p and "first 1 and last 1 bytes before its start" in p for p in problems), problems
    assert any("`b`" in p and "input modified" in p for p in problems), problems
    with pytest.raises(AssertionError, match="`a`"):
        arena.check()


@_params(C.ray_cases())
def test_per_ray_and_step_kernels(L, build):
    C.run_case(L, build(L), dev())


@_params(C.other_cases())
def test_gemm_adam_metrics(L, build):
    C.run_case(L, build(L), dev())


@pytest.mark.parametrize("precision,fwd_kernel", [(p, k) for p, ks in C.MLP_KERNELS.items() for k in ks],
                         ids=[f"{p}-k{k}" for p, ks in C.MLP_KERNELS.items() for k in ks])
def test_mlp_family(L, precision, fwd_kernel):
    """Every route (pts / viewdirs, embedded 63 | 27, embedded 57 | 3) and row count of one precision and forward kernel:
    pack, inference forward, training forward, backward, input gradient."""
    for case_id, build in C.mlp_cases(precision, fwd_kernel):
        try:
            C.run_case(L, build(L), dev())
        except AssertionError as e:
            raise AssertionError(f"{case_id}: {e}") from None


@pytest.mark.parametrize("precision", list(C.PRECISIONS))
def test_mlp_bwd_multi(L, precision):
    for case_id, build in C.mlp_multi_cases(precision):
        try:
            results = C.run_case(L, build(L), dev())
        except AssertionError as e:
            raise AssertionError(f"{case_id}: {e}") from None
        assert {f"j{j}_grad{k:02d}" for j in range(2) for k in range(24)} <= set(results)


@_params(C.one_call_cases())
def test_one_call_entries(L, build):
    """Two steps (or two calls on one frame) on a workspace of exactly the size query's bytes.  Losses, parameters and
    moments after the second step equal, bit for bit, the same calls on ordinary allocations: condition (b)."""
    results = C.run_case(L, build(L), dev())
    assert any(name.startswith(("loss", "plane_rgb")) for name in results)


def test_misaligned_float4_arrays_are_refused_and_nothing_is_written(L):
    """raw, g_raw, raw_out and feature_linear's weight / bias are accessed as float4: 4 bytes off a 16-byte boundary every
    entry answers PLNERF_EINVAL before its first launch -- guards intact, inputs unchanged, outputs still at the fill.  (The
    pointers are real memory of the full size.  The same calls are refused without a device in tests/test_alignment_abi.py;
    the aligned calls are the cases above.)"""
    for case_id, calls in C.misaligned_cases(L):
        try:
            C.run_refused(L, calls, dev())
        except AssertionError as e:
            raise AssertionError(f"{case_id}: {e}") from None
