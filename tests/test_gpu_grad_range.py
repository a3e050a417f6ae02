"""The 16-bit backward's launch scale over the gradient's range (include/plnerf_hip.h, "Backward of modes 1-4"; mlp_layout.h:
dzh_shift, whose table tests/test_mlp_bwd_plan.py sweeps on the CPU).  Every weight, bias, head and input gradient of a step
passes through that one power of two, derived from the workspace's max |g_raw| word at four kernel sites, and the word gets
there by three routes: the call's own pass, the caller's g_absmax candidates, and absmax_act when density_beta > 0.

The raw ABI on 1000 rows (125 rays of 8 samples, 63 | 27 channels: ragged against the 32-, 64-, 192- and 256-row tiles), network
closed_form_state_dict(3, False): plnerf_mlp_fwd with a saved state once per variant (once more with density_beta for that
route), then plnerf_mlp_bwd and plnerf_mlp_input_grad on one workspace per backward, workspace and outputs poisoned with NaN
before each.  tests/grad_range_cases.py holds the rows, the cotangents and the float64 yardstick.

  a. test_anchor_against_the_oracle       the base cotangent c against float64 autograd at the bounds test_gpu_parity.py asserts.
  b. test_homogeneity_bit_for_bit         g_raw = ldexp(c, k): every output is ldexp(output at k = 0, k), bit for bit, by each route.
  c. test_low_end_against_the_oracle      max |g_raw| = 2^-123, 2^-125, 2^-126 against the yardstick; 2^-135: finite outputs.
  d. test_two_jobs_two_exponents          plnerf_mlp_bwd_multi with launch exponents 80 apart.
  e. test_wide_range_inside_one_launch    rows from 2^-25 to 1 in one launch, against the yardstick at the bounds of (a).

Nothing non-finite is fed to a kernel.  Each part prints its figures on GRANGE lines (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import grad_range_cases as C
from gpu_support import P, dev, g, make_net  # noqa: F401
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu

KERNELS = {"auto": 0, "rr": 1, "pp": 2}      # PLNERF_FWD_KERNEL_*
# every training variant of the 16-bit modes (as test_gpu_encoding.SIXTEEN_BIT with role "train": there is no register-resident
# training forward in plain bf16), both saved-plane layouts among them, and the exact-fp32 kernels as the control: no scale
VARIANTS = [("fp32", "auto")] + [(mode, kernel) for mode in ("f16x3", "bf16x3", "f16", "bf16") for kernel in ("rr", "pp")
                                 if (mode, kernel) != ("bf16", "rr")]
ids = lambda v: "-".join(v)
SHIFTS = (-60, -24, -1, 1, 24, 60, 100)
ROUTES = ("own pass", "g_absmax", "density")
XC, DC = orc.XYZ_CH, orc.DIR_CH      # 63 | 27
_STATES, _WORKSPACES = {}, {}


class State:
    """One variant's network and its training forward(s), built once and reused by all its backwards, and a workspace."""

    def __init__(self, P, mode, kernel, sd, pts, vd):
        from plnerf_amd import _lib as L
        self.L, self.mode, self.prec, self.n = L, mode, L.PRECISION[mode], pts.shape[0] * pts.shape[1]
        self.net = make_net(P, sd, mode)
        self.packed = self.net.packed_weights()
        self.params = list(self.net.parameters())
        self.names = [name for name, _ in self.net.named_parameters()]
        self.layout = L.lib().plnerf_mlp_saved_layout(self.prec, 0, KERNELS[kernel])
        pts_d, vd_d = g(pts.reshape(-1, 3).contiguous()), g(vd.contiguous())
        self.saved, self.raw = {}, {}
        for beta in (0.0, C.DENSITY_BETA):
            raw = torch.full((self.n, 4), float("nan"), device=dev())
            saved = torch.full((L.lib().plnerf_mlp_saved_bytes(self.n, self.prec) // 4,), float("nan"), device=dev())
            L.check(L.lib().plnerf_mlp_fwd(L.dptr(self.packed), self.prec, L.dptr(pts_d), L.dptr(vd_d), None, XC, DC, self.n,
                                           pts.shape[1], 1.0, beta, L.dptr(raw), L.dptr(saved), KERNELS[kernel], L.stream()), "plnerf_mlp_fwd")
            torch.cuda.synchronize()
            assert torch.isfinite(raw).all(), (mode, kernel, beta)
            self.saved[beta], self.raw[beta] = saved, raw
        words = L.lib().plnerf_mlp_bwd_workspace_bytes(self.n, self.prec) // 4      # (0.3 GB whatever the rows: one per size for all states)
        if words not in _WORKSPACES:
            _WORKSPACES[words] = torch.empty(words, device=dev())
        self.ws = _WORKSPACES[words]

    def poisoned(self):
        self.ws.fill_(float("nan"))
        return ([torch.full(tuple(p.shape), float("nan"), device=dev()) for p in self.params],
                torch.full((self.n, XC + DC), float("nan"), device=dev()))

    def backward(self, g_raw, route="own pass"):
        """plnerf_mlp_bwd, then plnerf_mlp_input_grad on its workspace: the 24 parameter gradients and g_embedded, as numpy."""
        L = self.L
        assert g_raw.dtype == np.float32 and g_raw.shape == (self.n, 4) and np.isfinite(g_raw).all()
        grads, g_emb = self.poisoned()
        g_dev = g(torch.from_numpy(np.array(g_raw)))      # (a copy: the cached cotangents are read-only)
        cand = g(torch.from_numpy(C.absmax_candidates(g_raw))) if route == "g_absmax" else None
        beta = C.DENSITY_BETA if route == "density" else 0.0
        L.check(L.lib().plnerf_mlp_bwd(L.dptr(self.packed), self.prec, L.dptr(g_dev), L.dptr(cand, "g_absmax", torch.int32),
                                       0 if cand is None else cand.numel(), XC, DC, self.n, L.dptr(self.saved[beta]), self.layout,
                                       L.dptr(self.raw[beta]) if beta else None, beta, L.dptr(self.ws), L.ptr_table(grads, "grads"),
                                       None, L.stream()), "plnerf_mlp_bwd")
        L.check(L.lib().plnerf_mlp_input_grad(L.ptr_table(self.params, "params"), self.prec, XC, DC, self.n, L.dptr(self.ws),
                                              L.dptr(g_emb), L.stream()), "plnerf_mlp_input_grad")
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in grads + [g_emb]]


def state_of(P, variant):
    if variant not in _STATES:
        _STATES[variant] = State(P, *variant, C.state_dict(), *C.rows())
    return _STATES[variant]


def cotangent_of(mode, j_max=6):
    """The mode's cotangent: the rows gpu_support.ambiguous_rows flags at its amb are zeroed, and few are."""
    flagged = C.flagged(C.amb_of(mode))
    assert flagged.mean() <= C.AMB_CAP, (mode, int(flagged.sum()))
    return C.base(C.amb_of(mode), j_max)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def against_the_oracle(st, got, ref, factor=1.0, floor=0.0):
    """The 24 parameter gradients against `ref` x factor (float64) at the mode's bounds, relative to the reference's own
    max |g| (no absolute floor but `floor`): (worst error / max |g|, worst cosine, the tensors that miss)."""
    tol, min_cos = C.bounds_of(st.mode)
    worst, worst_cos, missed = 0.0, 1.0, []
    for name, a in zip(st.names, got):
        if not np.isfinite(a).all():
            missed.append((name, "non-finite entries"))
            continue
        err, cos = C.compare(a, ref[name] * factor, floor)
        worst, worst_cos = max(worst, err), min(worst_cos, cos)
        if (tol is not None and not err <= tol) or (min_cos is not None and not cos >= min_cos):
            missed.append((name, err, cos))
    return worst, worst_cos, missed


# ----------------------------------------------------------------------------- a. the anchor
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_anchor_against_the_oracle(P, variant):
    """k = 0: the base cotangent against float64 autograd on the oracle, at the bounds test_mlp_bf16_modes asserts (split modes
    1.5e-3 of max |g| per tensor and cosine >= 0.999999, plain modes cosine >= 0.99) and test_mlp_fwd_bwd_vs_oracle's 2e-5 for
    the exact-fp32 kernels -- what parts (b) and (d) compare with is itself right."""
    st = state_of(P, variant)
    got = st.backward(cotangent_of(st.mode))
    worst, worst_cos, missed = against_the_oracle(st, got[:-1], C.reference(C.amb_of(st.mode), "base"))
    print(f"GRANGE anchor {ids(variant)}: worst error / max |g| {worst:.3e}, worst cosine {worst_cos:.8f} (bounds {C.bounds_of(st.mode)})")
    assert np.isfinite(got[-1]).all(), "g_embedded"
    assert not missed, missed


# ----------------------------------------------------------------------------- b. homogeneity
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_homogeneity_bit_for_bit(P, variant, route):
    """The gradient is linear in the cotangent and a power of two is exact: g_raw = ldexp(c, k) puts the same bits into the
    scaled half planes for every k, the sums run on those, the un-scale is an exact power of two, and the fp32-side pieces (head
    launch, composed view layer, absmax_act's product) only multiply and add -- so all 24 parameter gradients and g_embedded
    are ldexp(result at k = 0, k), bit for bit, while nothing leaves the normal range.  Once per route of the max |g_raw|
    word; the routes that see the same g_raw (the call's own pass, g_absmax handed in) also agree with each other bit for bit.
    The exact-fp32 kernels carry no scale: the same holds for them trivially, every operation being a multiply or an add."""
    st = state_of(P, variant)
    c = cotangent_of(st.mode)
    names = st.names + ["g_embedded"]
    base = st.backward(c, route)
    assert all(np.isfinite(a).all() and np.abs(a).max() > 0 for a in base)
    if route == "g_absmax":
        own = st.backward(c)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(own, base)), "k = 0: own pass and g_absmax differ"
    broken = []
    for k in (SHIFTS if route != "density" else (-24, 24)):
        g_raw = np.ldexp(c, k)
        got = st.backward(g_raw, route)
        for name, a, b in zip(names, got, base):
            want = np.ldexp(b, k)
            if not np.array_equal(bits(a), bits(want)):
                rel = float(np.abs(a.astype(np.float64) - want).max() / np.abs(want.astype(np.float64)).max())
                broken.append((k, name, int((bits(a) != bits(want)).sum()), rel))
        if route == "g_absmax":
            own = st.backward(g_raw)
            broken += [(k, name, "own pass and g_absmax differ") for name, a, b in zip(names, own, got) if not np.array_equal(bits(a), bits(b))]
    print(f"GRANGE homogeneity {ids(variant)} {route}: {len(broken)} (k, tensor) pairs differ" + (f": {broken[:8]}" if broken else ""))
    assert not broken, broken[:8]


# ----------------------------------------------------------------------------- c. the low end
@pytest.mark.parametrize("p", (123, 125, 126, 135))
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_low_end_against_the_oracle(P, variant, p):
    """max |g_raw| exactly 2^-123 (the last value for which frexpf / ldexpf gave a finite scale, 2^127), 2^-125 and 2^-126 (normal
    numbers below it, where that scale was +inf: g inf = inf, or NaN for g = 0, and the saturating conversion made +-65,504 of
    them -- finite garbage out of a library entry without a status bit; dzh_shift caps the shift at 127 instead).  Reference: the
    float64 oracle gradient of g_raw 2^p times 2^-p -- float64 does not underflow there.  Bounds: those of (a), relative to the
    reference's own max |g|, plus 2^-126 absolute (one smallest normal) for fp32 outputs that go subnormal.  2^-135: max |g_raw|
    itself a subnormal; every output finite.

    Measured on an MI355X (LABNOTES.md, R16-1).  Before the cap: 2^-123 passed; at 2^-125 and 2^-126 every 16-bit variant was
    3.66e+6 x max |g| off, cosine -0.085.  With it: cosine 0.99999964 or better in the split modes, nothing beyond the allowance."""
    st = state_of(P, variant)
    cotangent_of(st.mode)
    g_raw, _ = C.low_end(C.amb_of(st.mode), p)
    got = st.backward(g_raw)
    finite = all(np.isfinite(a).all() for a in got)
    if p == 135:
        print(f"GRANGE low end {ids(variant)} max |g_raw| 2^-{p}: outputs finite {finite}")
        assert finite
        return
    ref = C.reference(C.amb_of(st.mode), "low", p)
    worst, worst_cos, missed = against_the_oracle(st, got[:-1], ref, 2.0 ** -p, 2.0 ** -126)
    whole = against_the_oracle(st, got[:-1], ref, 2.0 ** -p)[0]      # (reported: the error without the 2^-126 allowance)
    print(f"GRANGE low end {ids(variant)} max |g_raw| 2^-{p}: worst (error - 2^-126) / max |g| {worst:.3e} (error / max |g| {whole:.3e}), "
          f"worst cosine {worst_cos:.8f} (bounds {C.bounds_of(st.mode)}), g_embedded finite {bool(np.isfinite(got[-1]).all())}")
    assert not missed, missed
    assert finite


# ----------------------------------------------------------------------------- d. two jobs, two exponents
@pytest.mark.parametrize("with_absmax", (False, True), ids=("own pass", "g_absmax"))
@pytest.mark.parametrize("k0,k1", ((40, -40), (-40, 40)))
def test_two_jobs_two_exponents(P, k0, k1, with_absmax):
    """plnerf_mlp_bwd_multi in f16x3 on two networks (closed_form_state_dict(0 | 1), 1000 and 296 rows) whose cotangents are
    ldexp(c0, k0) and ldexp(c1, k1), 80 exponents apart: against the two separate plnerf_mlp_bwd calls exactly as
    test_gpu_step.py: test_merged_backward_equals_two_backwards compares (dz planes bit-identical; bias and head gradients equal
    or within 2e-6 of the job's own max |g|; everything within 2e-5), and each job against ldexp of its own single-job result
    at k = 0 with the same bounds.  A word read from the other job is off by 2^80.  (Kernel against kernel: no row is muted.)"""
    from plnerf_amd import _lib as L
    jobs = []
    for net_seed, n_rays, k in ((0, 125, k0), (1, 37, k1)):
        key = ("two jobs", net_seed)
        if key not in _STATES:
            _STATES[key] = State(P, "f16x3", "auto", C.state_dict(net_seed), *C.draw_rows(n_rays, net_seed, 30 + net_seed))
        st = _STATES[key]
        c = C.cotangent(st.n, 6, 40 + net_seed)
        jobs.append((st, np.ldexp(c, k), k, st.backward(c)[:-1]))
    prec = jobs[0][0].prec
    vp = lambda items: (ctypes.c_void_p * len(items))(*[None if x is None else x.value for x in items])
    single = []
    for st, g_raw, _, _ in jobs:
        grads = st.backward(g_raw)[:-1]
        single.append((st.ws.clone(), grads))
    ws = [torch.full_like(st.ws, float("nan")) for st, *_ in jobs]
    grads = [[torch.full(tuple(p.shape), float("nan"), device=dev()) for p in st.params] for st, *_ in jobs]
    g_dev = [g(torch.from_numpy(g_raw)) for _, g_raw, _, _ in jobs]
    am = [g(torch.from_numpy(C.absmax_candidates(g_raw))) if with_absmax else None for _, g_raw, _, _ in jobs]
    tails = torch.full((2, 4), -1.0, device=dev())
    L.check(L.lib().plnerf_mlp_bwd_multi(
        2, vp([L.dptr(st.packed) for st, *_ in jobs]), prec, vp([L.dptr(t) for t in g_dev]),
        vp([L.dptr(a, "g_absmax", torch.int32) for a in am]), (ctypes.c_int * 2)(*[0 if a is None else a.numel() for a in am]),
        XC, DC, (ctypes.c_int * 2)(*[st.n for st, *_ in jobs]), vp([L.dptr(st.saved[0.0]) for st, *_ in jobs]),
        (ctypes.c_int * 2)(*[st.layout for st, *_ in jobs]), None, 0.0, vp([L.dptr(w) for w in ws]),
        L.ptr_table([t for gr in grads for t in gr], "grads"), vp([ctypes.c_void_p(tails[j].data_ptr()) for j in range(2)]), L.stream()),
        "plnerf_mlp_bwd_multi")
    torch.cuda.synchronize()
    assert tails[:, 0].tolist() == [0.0, 0.0]
    worst = {"separate calls": 0.0, "ldexp of k = 0": 0.0}
    for j, (st, _, k, at_zero) in enumerate(jobs):
        ws_bytes = L.lib().plnerf_mlp_bwd_workspace_bytes
        n_dz = (ws_bytes(st.n, prec) - ws_bytes(0, prec) - 16 * st.n) // 4
        assert torch.equal(single[j][0][:n_dz].view(torch.int32), ws[j][:n_dz].view(torch.int32)), (j, "dz planes")
        merged = [t.cpu().numpy() for t in grads[j]]
        for what, ref in (("separate calls", single[j][1]), ("ldexp of k = 0", [np.ldexp(a, k) for a in at_zero])):
            for name, a, b in zip(st.names, ref, merged):
                assert np.isfinite(b).all(), (j, name)
                err = float(np.abs(a.astype(np.float64) - b).max() / (np.abs(a.astype(np.float64)).max() + 1e-300))
                worst[what] = max(worst[what], err)
                if name.endswith("bias") or name.startswith("rgb_linear"):
                    assert np.array_equal(a, b) or err <= 2e-6, (what, j, name, err)
                assert err <= 2e-5, (what, j, name, err)
    print(f"GRANGE two jobs, exponents {k0:+d} | {k1:+d}, g_absmax handed in {with_absmax}: dz planes bit-identical; worst gradient "
          f"difference / max |g| " + ", ".join(f"{w:.2e} ({what})" for what, w in worst.items()))


# ----------------------------------------------------------------------------- e. a wide range inside one launch
@pytest.mark.parametrize("variant", VARIANTS, ids=ids)
def test_wide_range_inside_one_launch(P, variant):
    """The same rows with per-row factors 2^-j, j uniform in 0..24, in ONE launch, against the float64 oracle at the bounds of
    (a): the large rows dominate every entry, and the small rows' half subnormals cost at most 2^-25 at a scale of 8-16."""
    st = state_of(P, variant)
    got = st.backward(cotangent_of(st.mode, 24))
    worst, worst_cos, missed = against_the_oracle(st, got[:-1], C.reference(C.amb_of(st.mode), "wide"))
    print(f"GRANGE wide range {ids(variant)}: worst error / max |g| {worst:.3e}, worst cosine {worst_cos:.8f} (bounds {C.bounds_of(st.mode)})")
    assert np.isfinite(got[-1]).all(), "g_embedded"
    assert not missed, missed
