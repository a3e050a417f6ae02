"""The fine pass's MLP forward over the rows it needs (include/experimental/plnerf_hip_unique.h; pl-nerf_amd/csrc/mlp_unique.hip,
mlp_unique_plan.h): a row whose position equals both neighbours' bit for bit, on its ray, is not evaluated -- its output is a
copy of the run's first row.

Forward, against plnerf_mlp_fwd on the same rows: `raw` bitwise equal for every row, in f16x3 and bf16x3, at 387 (129 x 3), 420
(60 x 7) and 448 (64 x 7) rows (the workgroup tile is 128 rows) under every row pattern of PATTERNS, with the workspace and
`saved` filled with NaN bit patterns before each call: every output finite, the range status word the plain call's, two runs
bit-identical, and n_eval / rows_u / src read back equal to a numpy model of the rule.

Backward: (unique forward, fold, plnerf_mlp_bwd_multi) against (plain forward, plnerf_mlp_bwd_multi).  With upstream gradients
that are zero on the interior rows all 24 gradients are bitwise equal.  With random gradients on every row both legs are within
6e-3 of max |reference| per tensor of the fp64 autograd reference (the bound and the rescaled heads of
tests/test_gpu_bwd_compact.py), the two legs differ by no more than that file allows between its legs (6e-3 of max
|reference|), and the unique leg is no further from fp64 than MARGIN times what the plain leg measures on the same case (plus
the fold's own fp32 rounding); the figures are printed.  MARGIN, reasoned: both errors are the half rounding (2^-11 relative)
of the dz planes, accumulated over the rows.  The plain leg rounds a run's L rows one by one, error^2 ~ sum of g_i^2; the
unique leg rounds the one folded row, error^2 ~ (sum of g_i)^2, which for the random gradients of this case has the same
expectation, L g^2.  So the two figures are two draws of the maximum, over a tensor's thousands of elements, of errors of one
distribution -- such maxima agree within tens of percent; a factor 2 separates that scatter from a leg that is systematically
worse.  The fold adds a run's rows in fp32: at most (L - 1) 2^-24 of the sum, L <= 30 here.

Whole step: TrainStep, 64 rays, 8 + 16 samples, three steps from the default initialisation (runs occur there: counted), route
on against route off: loss, both networks' weights, moments and .grad bitwise equal; with PLNERF_BWD_COMPACT=0 the step takes
the plain forward.
"""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

from gpu_support import P, assert_same_nvs_state, counting_calls, dev, g, make_net, same_bits, scene, size
from oracle import plnerf_oracle as orc
from run_args import nvs_args

pytestmark = pytest.mark.gpu

TOL = 6e-3
MARGIN = 2.0                     # unique leg's error against the plain leg's on the same case (docstring)
FOLD_ROUNDING = 29 * 2.0 ** -24  # the fold's fp32 sums over runs of at most 30 rows
SHAPES = ((129, 3), (60, 7), (64, 7))      # (rays, rows per ray): 387, 420, 448 rows


@pytest.fixture(scope="module")
def Fn(P):
    from plnerf_amd import functional
    return functional


@pytest.fixture(scope="module")
def L(P):
    from plnerf_amd import _lib
    return _lib


# ----------------------------------------------------------------------------- row patterns
def _runs(gen, R, S, lengths):
    """pts [R, S, 3]: every ray a sequence of runs of equal rows, run lengths cycled from `lengths` (cut at the ray's end)."""
    pts = torch.empty(R, S, 3)
    k = 0
    for r in range(R):
        s = 0
        while s < S:
            n = min(lengths[k % len(lengths)], S - s)
            pts[r, s:s + n] = torch.rand(3, generator=gen) * 4 - 2
            s += n
            k += 1
    return pts


def _next_up(x):
    return torch.from_numpy(np.nextafter(x.numpy(), np.float32(np.inf)))


def make_pattern(name, R, S, seed=0):
    gen = torch.Generator().manual_seed(1000 * seed + 7 * R + S)
    rnd = lambda: torch.rand(R, S, 3, generator=gen) * 4 - 2
    if name == "nothing repeated":
        return rnd()
    if name == "every row of a ray equal":
        return rnd()[:, :1].expand(R, S, 3).contiguous()
    if name == "runs of 1, 2, 3, 4":
        return _runs(gen, R, S, (1, 2, 3, 4, 4, 1, 3, 2, 2))
    if name == "run at a ray's first rows":
        p = rnd()
        p[:, :min(3, S)] = p[:, :1]
        return p
    if name == "run at a ray's last rows":
        p = rnd()
        p[:, -min(3, S):] = p[:, -1:]
        return p
    if name == "last row equals the next ray's first rows":
        p = rnd()
        n = min(3, S)
        p[1:, :n] = p[:-1, -1:].expand(R - 1, n, 3)      # (the directions differ: a missing same-ray test shows in the output)
        if S > 3:
            p[:, -2:] = p[:, -1:]
        return p
    if name == "one ulp and the sign of zero":
        p = _runs(gen, R, S, (3, 4, 5))
        q = p.clone().reshape(-1, 3)
        idx = torch.arange(1, q.shape[0], 2)
        comp = torch.randint(0, 3, (idx.numel(),), generator=gen)
        q[idx, comp] = _next_up(q[idx, comp])                 # every other row one ulp off in one component
        z = p.clone().reshape(-1, 3)
        z[:, 1] = 0.0
        z[idx, 1] = -0.0                                      # ... or equal but for the sign of a zero
        half = (torch.arange(R * S) // S) % 2 == 0
        return torch.where(half[:, None], q, z).reshape(R, S, 3)
    raise KeyError(name)


PATTERNS = ("nothing repeated", "every row of a ray equal", "runs of 1, 2, 3, 4", "run at a ray's first rows",
            "run at a ray's last rows", "last row equals the next ray's first rows", "one ulp and the sign of zero")


def model(pts, spr):
    """The rule in numpy: (n_eval, rows_u, src)."""
    bits = pts.reshape(-1, 3).numpy().view(np.uint32)
    n = bits.shape[0]
    k = np.arange(n) % spr
    eq = (bits[1:] == bits[:-1]).all(1)                       # eq[i]: row i + 1 equals row i
    interior = np.zeros(n, bool)
    interior[1:n - 1] = (k[1:n - 1] != 0) & (k[1:n - 1] != spr - 1) & eq[:-1] & eq[1:]
    ev = ~interior
    return int(ev.sum()), np.nonzero(ev)[0].astype(np.uint32), (np.cumsum(ev) - 1).astype(np.uint32)


# ----------------------------------------------------------------------------- the two entries, called directly
class Caller:
    def __init__(self, L, net):
        self.L, self.net, self.prec = L, net, L.PRECISION[net.precision]
        self.packed = net.packed_weights()

    def _status(self):
        torch.cuda.synchronize()
        return self.net.range_status(reset=True)

    def plain(self, pts, vd, spr, save):
        L, n = self.L, pts.shape[0]
        raw = torch.full((n, 4), float("nan"), device=dev())
        saved = torch.empty(L.lib().plnerf_mlp_saved_bytes(n, self.prec) // 4, device=dev()) if save else None
        L.check(L.lib().plnerf_mlp_fwd(L.dptr(self.packed), self.prec, L.dptr(pts), L.dptr(vd), None, 63, 27, n, spr, 1.0, 0.0,
                                       L.dptr(raw), L.dptr(saved), 0, L.stream()), "plnerf_mlp_fwd")
        return raw, self._status()

    def unique(self, pts, vd, spr, save):
        L, n = self.L, pts.shape[0]
        assert L.lib().plnerf_mlp_fwd_unique_served(self.prec, 0, 0, spr, n, int(save)) == 1
        nan32 = lambda nbytes: torch.full((nbytes // 4,), -1, dtype=torch.int32, device=dev()).view(torch.float32)      # 0xffffffff
        raw = nan32(16 * n).view(n, 4)
        ws = nan32(L.lib().plnerf_mlp_unique_workspace_bytes(n))
        saved = nan32(L.lib().plnerf_mlp_saved_bytes(n, self.prec)) if save else None
        L.check(L.lib().plnerf_mlp_fwd_unique(L.dptr(self.packed), self.prec, L.dptr(pts), L.dptr(vd), 63, 27, n, spr, 1.0, 0.0,
                                              L.dptr(raw), L.dptr(saved), 0, L.dptr(ws), L.stream()), "plnerf_mlp_fwd_unique")
        status = self._status()
        lo = L.UniqueLayout()
        L.check(L.lib().plnerf_mlp_unique_layout(n, ctypes.byref(lo)), "plnerf_mlp_unique_layout")
        words = ws.view(torch.int32).cpu().numpy().view(np.uint32)
        n_eval = int(words[lo.words // 4])
        return raw, status, (n_eval, words[lo.rows_u // 4:lo.rows_u // 4 + n_eval], words[lo.src // 4:lo.src // 4 + n]), ws, lo


def check_forward(caller, pts, vd, what, save=True, n_eval=None):
    R, S = pts.shape[:2]
    flat, dirs = g(pts.reshape(-1, 3).contiguous()), g(vd)
    want, status_plain = caller.plain(flat, dirs, S, save)
    got, status, listed, _, _ = caller.unique(flat, dirs, S, save)
    again = caller.unique(flat, dirs, S, save)[0]
    expect = model(pts, S)
    print(f"{what}: {R} x {S} rows, n_eval {listed[0]} (model {expect[0]})")
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got).all()), what
    assert listed[0] == expect[0] and np.array_equal(listed[1], expect[1]) and np.array_equal(listed[2], expect[2]), what
    if n_eval is not None:
        assert listed[0] == n_eval, (what, listed[0])
    assert same_bits(got, want), (what, int((got.view(torch.int32) != want.view(torch.int32)).any(1).sum()), "rows differ")
    assert same_bits(got, again), (what, "two runs differ")
    assert status == status_plain, (what, status, status_plain)


def directions(R, seed=0):
    gen = torch.Generator().manual_seed(50 + seed)
    return torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)


@pytest.fixture(scope="module")
def callers(P, L):
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = Caller(L, make_net(P, orc.closed_form_state_dict(1, False), precision))
        return made[precision]
    return get


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_forward_is_the_plain_forward_bit_for_bit(callers, precision, shape):
    R, S = shape
    for name in PATTERNS:
        check_forward(callers(precision), make_pattern(name, R, S), directions(R), f"{precision}, {name}")
    # (the inference kernel: no saved state)
    check_forward(callers(precision), make_pattern("runs of 1, 2, 3, 4", R, S, seed=1), directions(R, 1), f"{precision}, no saved state",
                  save=False)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_tile_edges_and_a_single_ray(callers, precision):
    c = callers(precision)
    # 64 rays of 7 equal rows: two evaluated rows per ray, n_eval = 128 = one workgroup tile exactly
    p = make_pattern("every row of a ray equal", 64, 7)
    check_forward(c, p, directions(64), f"{precision}, n_eval 128", n_eval=128)
    # ... and one ray with a run of six and a last row of its own: 129
    p = p.clone()
    p[5, 6] = p[5, 6] + 1.0
    check_forward(c, p, directions(64), f"{precision}, n_eval 129", n_eval=129)
    for S, lengths in ((7, (3, 4)), (192, (65, 126, 1)), (3, (3,))):
        check_forward(c, _runs(torch.Generator().manual_seed(S), 1, S, lengths), directions(1, 2), f"{precision}, a single ray of {S}")


# ----------------------------------------------------------------------------- backward
def decisive_state_dict(seed, pts, vd, margin=1.5):
    """tests/test_gpu_bwd_compact.py's recipe: closed_form_state_dict(seed, True) with every hidden unit's bias moved so that over
    the rows the unit is on everywhere or off everywhere, and the heads rescaled to a scene-like range."""
    F = torch.nn.functional
    sd = {k: v.double().clone() for k, v in orc.closed_form_state_dict(seed, True).items()}
    gen = torch.Generator().manual_seed(1000 + seed)
    R, S = pts.shape[:2]
    enc_xyz = orc.positional_encoding(pts.reshape(-1, 3), orc.XYZ_FREQS)
    enc_dir = orc.positional_encoding(vd[:, None, :].expand(R, S, 3).reshape(-1, 3), orc.DIR_FREQS)

    def decide(z, key):
        lo, hi = z.min(0).values, z.max(0).values
        sign = torch.where(torch.rand(z.shape[1], generator=gen) < 0.5, 1.0, -1.0).double()
        shift = -0.5 * (hi + lo) + sign * (margin * 0.5 * (hi - lo) + 0.05)
        sd[key] += shift
        return z + shift
    h = enc_xyz
    for i in range(orc.DEPTH):
        z = decide(F.linear(h, sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]), f"pts_linears.{i}.bias")
        h = F.relu(z)
        if i == orc.SKIP_AFTER:
            h = torch.cat([enc_xyz, h], -1)
    feat = F.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
    zv = decide(F.linear(torch.cat([feat, enc_dir], -1), sd["views_linears.0.weight"], sd["views_linears.0.bias"]), "views_linears.0.bias")
    sigma = F.linear(h, sd["alpha_linear.weight"], sd["alpha_linear.bias"])
    rgb = F.linear(F.relu(zv), sd["rgb_linear.weight"], sd["rgb_linear.bias"])
    k_s = 0.06 / float(sigma.std())
    sd["alpha_linear.weight"] *= k_s
    sd["alpha_linear.bias"] = (sd["alpha_linear.bias"] - sigma.mean()) * k_s + 0.3
    k_c = 1.5 / rgb.std(0)
    sd["rgb_linear.weight"] *= k_c[:, None]
    sd["rgb_linear.bias"] = (sd["rgb_linear.bias"] - rgb.mean(0)) * k_c
    return {k: v.float() for k, v in sd.items()}


class Legs:
    """One network's training forward over the same rows twice -- the unique-row route and the plain one -- kept for several
    backwards, and the fp64 reference."""

    def __init__(self, P, Fn, precision, R=7, S=64, seed=0):
        gen = torch.Generator().manual_seed(31 + seed)
        self.pts = _runs(gen, R, S, (1, 5, 2, 30, 3, 1, 4, 12)) * 1.25
        self.vd = directions(R, seed)
        self.n, self.S = R * S, S
        sd = decisive_state_dict(seed, self.pts.double(), self.vd.double())
        self.net = make_net(P, sd, precision)
        self.interior = torch.from_numpy(np.setdiff1d(np.arange(self.n), model(self.pts, S)[1]))
        assert 100 < self.interior.numel() < self.n - 100
        self.legs = {}
        for name, fine in (("unique", True), ("plain", False)):
            Fn.MLP_TAPE, Fn.FINE_QUERY = Fn.MlpTape(), fine
            try:
                self.net.query(g(self.pts), g(self.vd))
                (out,) = Fn.MLP_TAPE.outs
            finally:
                Fn.MLP_TAPE, Fn.FINE_QUERY = None, False
            ctx = out.grad_fn
            assert (ctx.unique_ws is not None) == fine
            self.legs[name] = (out, ctx, ctx.saved_acts, ctx.unique_ws)
        assert same_bits(self.legs["unique"][0], self.legs["plain"][0])
        named = list(self.net.named_parameters())
        self.names = [next(k for k, q in named if q is p) for p in self.net.param_list()]
        self.sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        emb = torch.cat([orc.positional_encoding(self.pts.reshape(-1, 3).double(), orc.XYZ_FREQS),
                         orc.positional_encoding(self.vd.double()[:, None].expand(R, S, 3).reshape(-1, 3), orc.DIR_FREQS)], -1)
        self.raw64 = orc.nerf_mlp(self.sd64, emb)
        self.cot = torch.randn(self.n, 4, generator=gen)

    def backward(self, Fn, leg, g_raw):
        out, ctx, saved, ws = self.legs[leg]
        ctx.saved_acts, ctx.unique_ws = saved, ws      # (a used-up state is put back first)
        (grads,) = Fn.mlp_backward_multi([out], [g(g_raw)])
        torch.cuda.synchronize()
        return dict(zip(self.names, (t.clone() for t in grads)))

    def reference(self, g_raw):
        grads = torch.autograd.grad((self.raw64 * g_raw.double()).sum(), [self.sd64[k] for k in self.names], retain_graph=True)
        return dict(zip(self.names, grads))


def worst_error(got, ref):
    return max(float((got[k].cpu().double() - r).abs().max()) / float(r.abs().max()) for k, r in ref.items())


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_backward_through_the_fold(P, Fn, precision):
    legs = Legs(P, Fn, precision)
    # zero on the interior rows (what the quadrature hands a row between zero-length intervals): bit for bit
    g_raw = legs.cot.clone()
    g_raw[legs.interior] = 0.0
    a, b = legs.backward(Fn, "unique", g_raw), legs.backward(Fn, "plain", g_raw)
    again = legs.backward(Fn, "unique", g_raw)
    assert len(a) == 24 and all(bool(torch.isfinite(t).all()) for t in a.values())
    for k in a:
        assert same_bits(a[k], b[k]), (precision, k, "unique and plain legs differ", float((a[k] - b[k]).abs().max()))
        assert same_bits(a[k], again[k]), (precision, k, "two runs differ")
    # random on every row: the fold sums a run's rows onto its first row
    g_raw = legs.cot
    ref = legs.reference(g_raw)
    a, b = legs.backward(Fn, "unique", g_raw), legs.backward(Fn, "plain", g_raw)
    e_unique, e_plain = worst_error(a, ref), worst_error(b, ref)
    diff = max(float((a[k] - b[k]).abs().max()) / float(ref[k].abs().max()) for k in a)
    print(f"{precision}, random gradients on {legs.n} rows ({legs.interior.numel()} interior): worst error / max |ref| unique "
          f"{e_unique:.2e}, plain {e_plain:.2e}; unique vs plain {diff:.2e}")
    assert e_plain <= TOL, (precision, e_plain)
    assert e_unique <= TOL, (precision, e_unique)
    assert diff <= TOL, (precision, diff)
    assert e_unique <= MARGIN * e_plain + FOLD_ROUNDING, (precision, e_unique, e_plain)


# ----------------------------------------------------------------------------- the whole step
def _train_step(P, seed=11, **flags):
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "exp"))
    args = nvs_args(d, "f16x3", N_rand=64, N_samples=8, N_importance=16)
    torch.manual_seed(seed)      # the default initialisation, the same for every leg
    kw, _, start, _, opt, opt_c = P.create_nerf(args, device=dev())
    return P.TrainStep(args, kw, opt, opt_c, start=start, distributed=False, seed=5, range_check_every=0, **flags)


def _three_steps(P, Fn, ts):
    H, W, _ = size(256)
    poses, images, K = scene(P, 4, H, W, seed=3)
    images = g(images)
    with counting_calls() as lib:      # (which forward entry the Python route called)
        log = [ts.step_view(H, W, K, poses[k % 4][:3, :4], images[k % 4], near=2.0, far=6.0, n_rand=64) for k in range(3)]
        torch.cuda.synchronize()
    return log, lib.calls.count("plnerf_mlp_fwd_unique")


def test_whole_step_is_bit_identical(P, Fn):
    on = _train_step(P)
    log_on, calls_on = _three_steps(P, Fn, on)
    Fn.FWD_UNIQUE = False
    try:
        off = _train_step(P)
        log_off, calls_off = _three_steps(P, Fn, off)
    finally:
        Fn.FWD_UNIQUE = True
    assert calls_on == 3 and calls_off == 0
    for (la, pa), (lb, pb) in zip(log_on, log_off):
        assert bool(torch.isfinite(la)) and torch.equal(la, lb) and torch.equal(pa, pb), (float(la), float(lb))
    assert_same_nvs_state(on, off, "unique-row forward on / off")
    # ... and once as ONE library call per step (step_common.h takes the same route for the fine pass, and folds)
    one = _train_step(P, one_call=True)
    log_one, _ = _three_steps(P, Fn, one)
    assert one.one_call_steps == 3
    for (la, pa), (lb, pb) in zip(log_one, log_off):
        assert torch.equal(la, lb) and torch.equal(pa, pb), (float(la), float(lb))
    assert_same_nvs_state(one, off, "one-call step with the unique-row forward / plain Python route")
    # the dense backward would read planes nobody wrote: the step takes the plain forward, and is the same step again
    found = os.environ.get("PLNERF_BWD_COMPACT")
    os.environ["PLNERF_BWD_COMPACT"] = "0"
    try:
        dense = _train_step(P)
        log_dense, calls_dense = _three_steps(P, Fn, dense)
    finally:
        if found is None:
            del os.environ["PLNERF_BWD_COMPACT"]
        else:
            os.environ["PLNERF_BWD_COMPACT"] = found
    assert calls_dense == 0
    assert all(bool(torch.isfinite(l)) for l, _ in log_dense)


def test_runs_occur_in_that_step(P, Fn):
    """The fine pass of the step above does hold interior rows (else the comparison would be of the plain forward with itself):
    counted from the depths the render leaves behind."""
    import sys
    render_module = sys.modules["plnerf_amd.render"]
    from gpu_support import stage_tap
    ts = _train_step(P)
    H, W, _ = size(256)
    poses, images, K = scene(P, 4, H, W, seed=3)
    with stage_tap(render_module) as tap:
        ts.step_view(H, W, K, poses[0][:3, :4], g(images)[0], near=2.0, far=6.0, n_rand=64)
    z = tap["z_fine"].detach().cpu()
    eq = z[:, 1:] == z[:, :-1]
    interior = int((eq[:, 1:] & eq[:, :-1]).sum())
    print(f"interior rows in the first step: {interior} of {z.numel()}")
    assert interior > 0
