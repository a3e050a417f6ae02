"""plnerf_fine_epilogue_const_bwd (include/plnerf_hip_conststep.h) on a real MI355X: the backward of the constant-mode
final stage as one launch equals, bit for bit, the sequence it replaces on the forward outputs of
plnerf_fine_epilogue_const --

    plnerf_sample_const_bwd(bins, weights[:, 1:-1].contiguous(), u, inds, g_hyp)  ->  g_in [R, S-2]
    torch: zeros [R, S], the slice assignment, the optional add with g_weights
    plnerf_quad_bwd(PLNERF_MODE_CONSTANT, ..., that sum)                           ->  g_raw, max |g_raw| per workgroup

(functional.FineEpilogueFn.backward's constant branch) -- in g_raw and in every absmax word.  No tolerance: both sides run the
same device functions in the same order (csrc/ray_bwd_dev.h), built with -ffp-contract=off.

Shapes: S in {3, 4, 66, 67, 130} -- one interior weight, and both sides of the 64-lane scan boundary of the sampler's
n = S - 2 and of the quadrature's n = S; N in {1, 5, 64, 65}; R in {1, 5, 8}, which leave dead waves in the last workgroup of
4 rays."""
import pytest
import torch

from gpu_support import dev, g, quad_case

pytestmark = pytest.mark.gpu
GROUP = 4      # PLNERF_QUAD_RAYS_PER_GROUP


@pytest.fixture(scope="module")
def L():
    import plnerf_amd      # noqa: F401
    from plnerf_amd import _lib
    return _lib


def _forward(L, c, N, white, shared_u):
    """plnerf_fine_epilogue_const on the case: what the backward is handed."""
    R, S = c["z"].shape
    d = dev()
    rgb = torch.empty(R, 3, device=d)
    disp, acc, depth, z_std = (torch.empty(R, device=d) for _ in range(4))
    w, bins = torch.empty(R, S, device=d), torch.empty(R, S - 1, device=d)
    hyp, inds = torch.empty(R, N, device=d), torch.empty(R, N, device=d, dtype=torch.int64)
    u = c["u"][0].contiguous() if shared_u else c["u"]
    L.check(L.lib().plnerf_fine_epilogue_const(
        L.dptr(c["raw"]), L.dptr(c["z"]), L.dptr(c["near"]), L.dptr(c["far"]), L.dptr(c["d"]), L.dptr(c["noise"]), L.dptr(u),
        0 if shared_u else N, 0, 0, 0, R, S, N, int(white), L.dptr(rgb), L.dptr(disp), L.dptr(acc), L.dptr(depth), L.dptr(w),
        L.dptr(bins), L.dptr(hyp), L.dptr(inds, "inds", torch.int64), None, L.dptr(z_std), L.stream()),
        "plnerf_fine_epilogue_const")
    return dict(w=w, bins=bins, inds=inds, u=u, stride=0 if shared_u else N, hyp=hyp)


def _absmax(R):
    # (a pattern no float maximum writes: every word must be overwritten)
    return torch.full(((R + GROUP - 1) // GROUP,), -1, device=dev(), dtype=torch.int32)


def _separate(L, c, f, N, white, cot):
    """The yardstick: the three steps of FineEpilogueFn.backward's constant branch."""
    R, S = c["z"].shape
    g_w = cot["g_weights"]
    if cot["g_hyp"] is not None:
        g_in = torch.empty(R, S - 2, device=dev())
        L.check(L.lib().plnerf_sample_const_bwd(
            L.dptr(f["bins"]), L.dptr(f["w"][:, 1:-1].contiguous()), L.dptr(f["u"]), f["stride"],
            L.dptr(f["inds"], "inds", torch.int64), L.dptr(cot["g_hyp"]), R, S - 1, N, L.dptr(g_in), L.stream()),
            "plnerf_sample_const_bwd")
        g_s = torch.zeros(R, S, device=dev())
        g_s[:, 1:-1] = g_in
        g_w = g_s if g_w is None else g_w + g_s
    g_raw, absmax = torch.empty(R, S, 4, device=dev()), _absmax(R)
    L.check(L.lib().plnerf_quad_bwd(
        L.dptr(c["raw"]), L.dptr(c["z"]), L.dptr(c["near"]), L.dptr(c["far"]), L.dptr(c["d"]), L.dptr(c["noise"]), R, S,
        L.MODE["constant"], L.COLOR["midpoint"], int(white), 0, L.dptr(cot["g_rgb"]), L.dptr(cot["g_depth"]),
        L.dptr(cot["g_acc"]), L.dptr(g_w), None, None, L.dptr(g_raw), L.dptr(absmax, "absmax", torch.int32), L.stream()),
        "plnerf_quad_bwd")
    return g_raw, absmax


def _fused(L, c, f, N, white, cot, want_absmax=True):
    R, S = c["z"].shape
    g_raw, absmax = torch.empty(R, S, 4, device=dev()), (_absmax(R) if want_absmax else None)
    L.check(L.lib().plnerf_fine_epilogue_const_bwd(
        L.dptr(c["raw"]), L.dptr(c["z"]), L.dptr(c["near"]), L.dptr(c["far"]), L.dptr(c["d"]), L.dptr(c["noise"]),
        L.dptr(f["w"]), L.dptr(f["bins"]), L.dptr(f["u"]), f["stride"], L.dptr(f["inds"], "inds", torch.int64), R, S, N,
        int(white), L.dptr(cot["g_rgb"]), L.dptr(cot["g_depth"]), L.dptr(cot["g_acc"]), L.dptr(cot["g_weights"]),
        L.dptr(cot["g_hyp"]), L.dptr(g_raw), L.dptr(absmax, "absmax", torch.int32), L.stream()),
        "plnerf_fine_epilogue_const_bwd")
    return g_raw, absmax


def _case(R, S, N, seed, with_noise):
    raw, z, near, far, d, noise = quad_case(R, S, seed)
    gen = torch.Generator().manual_seed(31 * S + N)
    c = dict(raw=raw, z=z, near=near.reshape(-1), far=far.reshape(-1), d=d, noise=0.5 * noise if with_noise else None,
             u=torch.rand(R, N, generator=gen))
    cot = dict(g_rgb=torch.randn(R, 3, generator=gen), g_depth=torch.randn(R, generator=gen),
               g_acc=torch.randn(R, generator=gen), g_weights=0.1 * torch.randn(R, S, generator=gen),
               g_hyp=torch.randn(R, N, generator=gen))
    return c, cot


def _to_dev(d):
    return {k: (None if v is None else g(v).contiguous()) for k, v in d.items()}


def _check(L, c, cot, N, white, shared_u, what):
    c, cot = _to_dev(c), _to_dev(cot)
    f = _forward(L, c, N, white, shared_u)
    ref_raw, ref_max = _separate(L, c, f, N, white, cot)
    raw_, max_ = _fused(L, c, f, N, white, cot)
    torch.cuda.synchronize()
    assert torch.equal(ref_raw.view(torch.int32), raw_.view(torch.int32)), \
        (what, "g_raw", float((ref_raw - raw_).abs().nan_to_num(1e30).max()))
    assert torch.equal(ref_max, max_), (what, "absmax", ref_max.tolist(), max_.tolist())
    assert not bool((max_ == -1).any()), (what, "an absmax word was left unwritten")
    return f, ref_raw


@pytest.mark.parametrize("N", [1, 5, 64, 65])
@pytest.mark.parametrize("S", [3, 4, 66, 67, 130])
def test_one_launch_equals_the_separate_sequence(L, S, N):
    """Every R; the draws per ray and as one shared row, noise given and NULL, both backgrounds -- spread over the cases."""
    for R in (1, 5, 8):
        k = S + N + R
        white, shared_u, with_noise = k % 2 == 0, (k // 2) % 2 == 0, (k // 4) % 2 == 0
        c, cot = _case(R, S, N, 500 + S + R, with_noise)
        _check(L, c, cot, N, white, shared_u, f"S={S} N={N} R={R} white={white} shared_u={shared_u} noise={with_noise}")


@pytest.mark.parametrize("shared_u", [False, True])
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("white", [0, 1])
def test_draw_layouts_noise_and_background(L, white, with_noise, shared_u):
    c, cot = _case(5, 67, 5, 77, with_noise)
    _check(L, c, cot, 5, white, shared_u, f"white={white} noise={with_noise} shared_u={shared_u}")


@pytest.mark.parametrize("mask", range(16))
def test_every_optional_cotangent_given_and_null(L, mask):
    """g_depth, g_acc, g_weights, g_hyp: each given or NULL.  With g_hyp NULL the call must be plain plnerf_quad_bwd."""
    S, N, R = 67, 5, 5
    c, cot = _case(R, S, N, 91, True)
    for bit, name in enumerate(("g_depth", "g_acc", "g_weights", "g_hyp")):
        if not mask & (1 << bit):
            cot[name] = None
    _check(L, c, cot, N, 1, False, f"mask={mask:04b}")


def test_absmax_is_optional(L):
    c, cot = _case(5, 66, 5, 13, False)
    c, cot = _to_dev(c), _to_dev(cot)
    f = _forward(L, c, 5, 0, False)
    ref_raw, _ = _separate(L, c, f, 5, 0, cot)
    raw_, _ = _fused(L, c, f, 5, 0, cot, want_absmax=False)
    assert torch.equal(ref_raw, raw_)


def test_hard_rows(L):
    """Rows that take the sampler's special cases, at (16, 24): no density at all (zero weights, every cdf interval under
    1e-5: the inactive branch); one dominant sample (many draws land in one bin); repeated depths; draws at the cdf's ends."""
    S, N, R = 16, 24, 8
    c, cot = _case(R, S, N, 77, False)
    c["raw"][0, :, 3] = -5.0
    c["raw"][1, :, 3] = -5.0
    c["raw"][2, :, 3] = -5.0
    c["raw"][2, 6, 3] = 1e6                  # one opaque sample: the cdf is a plateau on both sides of one step
    c["raw"][3, :, 3] = 0.0                  # exact zeros
    c["z"][4, 5:9] = c["z"][4, 5]            # repeated depths: zero-length intervals and equal bins
    c["z"][5, :] = c["z"][5, 0]
    c["u"][0, :4] = torch.tensor([0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24])
    c["u"][2, :4] = torch.tensor([0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24])
    f, _ = _check(L, c, cot, N, 1, False, "hard rows")
    w = f["w"]
    assert float(w[0].abs().max()) == 0.0 and float(w[1].abs().max()) == 0.0 and float(w[2, 6]) == 1.0
    # the dominant row really gathers its draws in one bin
    assert int(torch.bincount(f["inds"][2].reshape(-1)).max()) >= N // 2


def test_no_rays_launch_nothing(L):
    """R = 0: PLNERF_OK with every pointer NULL -- nothing can have been dereferenced or launched."""
    assert L.lib().plnerf_fine_epilogue_const_bwd(None, None, None, None, None, None, None, None, None, 0, None, 0, 16, 8, 0,
                                                  None, None, None, None, None, None, None, L.stream()) == 0
    torch.cuda.synchronize()
