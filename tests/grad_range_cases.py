"""The CPU side of tests/test_gpu_grad_range.py, each piece written once: the rows, the cotangents and the float64 yardstick
(tests/test_grad_range_host.py checks them without a GPU).

Rows: 125 rays of 8 samples = 1000 rows (ragged against the 32-, 64-, 192- and 256-row tiles), positions uniform in
[-2.5, 2.5]^3 as in test_gpu_parity.py: test_mlp_bf16_modes, network closed_form_state_dict(3, False).  A uniform draw is no
use here: gpu_support.ambiguous_rows at that test's `amb` flags 61-66 % of such rows at bf16x3's 5e-5 and 8-11 % at f16x3's
5e-6 (seeds 0..2, three box sizes; 2,176 ReLU units per row, each within amb of zero with probability ~ 1e-4 amb / 5e-5), and
a cotangent that is mostly zeros tests little.  So every ray draws 64 candidate positions and keeps its first 8 that the fp64
oracle does NOT flag at the widest amb (5e-5): still uniform over the part of the box where every mode takes the oracle's ReLU
branches, and the same rows serve every mode.  ambiguous_rows is then asked again per mode, its rows are zeroed in the cotangent
and at most AMB_CAP of them may be flagged -- by construction none is.

Cotangents: per row a factor 2^-j (j uniform in 0..j_max), per element a magnitude in [0.5, 1) and a random sign, float32.
ldexp of such an array by k is exact while 2^(k - j_max - 1) is a normal number."""
import functools

import numpy as np
import torch

from gpu_support import ambiguous_rows
from oracle import plnerf_oracle as orc

N_RAYS, SPR = 125, 8
N_ROWS = N_RAYS * SPR
NET_SEED = 3
AMB = {"bf16x3": 5e-5, "f16x3": 5e-6}      # test_mlp_bf16_modes: plain 16-bit operands and fp32 have no sharp comparison / need none
AMB_CAP = 0.05
CANDIDATES = 64
DENSITY_BETA = 10.0


def amb_of(mode):
    return AMB.get(mode, 0.0)


def state_dict(seed=NET_SEED):
    return orc.closed_form_state_dict(seed, False)


def draw_rows(n_rays, net_seed, seed):
    """(pts [n_rays, SPR, 3], viewdirs [n_rays, 3]) float32: per ray the first SPR of CANDIDATES uniform positions that the fp64
    oracle does not flag at the widest amb."""
    gen = torch.Generator().manual_seed(seed)
    cand = (torch.rand(n_rays, CANDIDATES, 3, generator=gen) * 2 - 1) * 2.5
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1)
    ok = ~ambiguous_rows(state_dict(net_seed), cand, vd, max(AMB.values())).reshape(n_rays, CANDIDATES)
    assert int(ok.sum(-1).min()) >= SPR, ("a ray with fewer than SPR unambiguous candidates", int(ok.sum(-1).min()))
    first = torch.argsort((~ok).to(torch.int8), dim=-1, stable=True)[:, :SPR]      # the unflagged ones first, in drawing order
    pts = torch.gather(cand, 1, first[..., None].expand(n_rays, SPR, 3)).contiguous()
    return pts, vd


@functools.lru_cache(maxsize=None)
def rows():
    return draw_rows(N_RAYS, NET_SEED, 20)


@functools.lru_cache(maxsize=None)
def flagged(amb):
    """ambiguous_rows of the rows at a mode's amb (amb_of): bool [N_ROWS]."""
    pts, vd = rows()
    return ambiguous_rows(state_dict(), pts, vd, amb).numpy()


def cotangent(n_rows, j_max, seed):
    """float32 [n_rows, 4]: 2^-j per row (j uniform in 0..j_max) x a magnitude in [0.5, 1) x a random sign."""
    rng = np.random.default_rng(seed)
    j = rng.integers(0, j_max + 1, (n_rows, 1))
    c = np.ldexp(rng.uniform(0.5, 1.0, (n_rows, 4)).astype(np.float32), -j) * rng.choice(np.float32([-1.0, 1.0]), (n_rows, 4))
    return c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def base(amb, j_max=6):
    """The base cotangent c (j_max 6), or the wide one of part (e) (j_max 24), with the rows flagged at `amb` zeroed."""
    c = cotangent(N_ROWS, j_max, 100 + j_max) * ~flagged(amb)[:, None]
    c.setflags(write=False)
    return c


def unit_max(c):
    """c / max |c| in float64, rounded to float32: the largest magnitude is exactly 1."""
    c1 = (c.astype(np.float64) / np.abs(c).max()).astype(np.float32)
    assert np.abs(c1).max() == 1.0
    return c1


def low_end(amb, p):
    """Part (c): (g_raw float32 with max |g_raw| exactly 2^-p, the float64 array g_raw 2^p) -- the second is what the yardstick
    differentiates, so the rounding of g_raw's small rows to fp32 subnormals is in the reference too."""
    g_raw = np.ldexp(unit_max(base(amb)).astype(np.float64), -p).astype(np.float32)
    assert np.abs(g_raw).max() == np.float32(2.0) ** -p and np.isfinite(g_raw).all()
    return g_raw, np.ldexp(g_raw.astype(np.float64), p)


def absmax_candidates(g_raw):
    """max |g_raw| as plnerf_quad_bwd's absmax_out hands it over: the maxima of groups of 32 values, as fp32 bit patterns
    (test_gpu_step.py: test_merged_backward_equals_two_backwards builds them so, on the device)."""
    flat = np.abs(np.asarray(g_raw, np.float32)).reshape(-1)
    flat = np.concatenate([flat, np.zeros((-flat.size) % 32, np.float32)])
    return np.ascontiguousarray(flat.reshape(-1, 32).max(-1)).view(np.int32)


def embedded64(pts, vd):
    n_rays, spr = pts.shape[:2]
    return torch.cat([orc.positional_encoding(pts.reshape(-1, 3).double(), orc.XYZ_FREQS),
                      orc.positional_encoding(vd.double()[:, None].expand(n_rays, spr, 3).reshape(-1, 3), orc.DIR_FREQS)], -1)


def oracle_grads(cot64):
    """float64 autograd of sum(raw * cot64) on the oracle network at the rows: {parameter name: gradient}."""
    sd = {k: v.double().requires_grad_(True) for k, v in state_dict().items()}
    raw = orc.nerf_mlp(sd, embedded64(*rows()))
    (raw * torch.from_numpy(np.ascontiguousarray(cot64, dtype=np.float64))).sum().backward()
    return {k: v.grad.numpy() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def reference(amb, kind, p=0):
    """The yardstick of one cotangent, computed once: kind "base" (part a), "wide" (part e) or "low" (part c at max |g_raw| =
    2^-p: the gradient of g_raw 2^p, which the caller multiplies by 2^-p in float64)."""
    if kind == "low":
        return oracle_grads(low_end(amb, p)[1])
    return oracle_grads(base(amb, 24 if kind == "wide" else 6).astype(np.float64))


# the bounds test_gpu_parity.py asserts on the 24 parameter gradients against the oracle: test_mlp_bf16_modes (split modes:
# 1.5e-3 of max |g| per tensor and cosine >= 0.999999; plain modes: cosine >= 0.99) and test_mlp_fwd_bwd_vs_oracle (fp32: 2e-5)
def bounds_of(mode):
    """(error / max |g| per tensor or None, cosine per tensor or None)"""
    if mode == "fp32":
        return 2e-5, None
    return (1.5e-3, 0.999999) if mode in ("bf16x3", "f16x3") else (None, 0.99)


def compare(got, ref, floor=0.0):
    """Per tensor, in float64: (worst excess of |got - ref| over `floor`, as a share of the REFERENCE's own max |g|; cosine)."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    err = np.maximum(np.abs(got - ref) - floor, 0.0).max() / np.abs(ref).max()
    cos = float(got @ ref / (np.linalg.norm(got) * np.linalg.norm(ref)))
    return float(err), cos
