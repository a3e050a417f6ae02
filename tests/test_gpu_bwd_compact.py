"""The 16-bit modes' MLP backward over the LIVE rows only (pl-nerf_amd/csrc/mlp_bwd_plan.h, "live rows"; mlp_live.hip):
rows whose upstream gradient is exactly (0, 0, 0, 0) are listed out before dgrad, the dz planes hold the live rows
compacted, the weight-gradient stage gathers its saved rows through the list.

One training forward per (mode, row count) through NeRF.query, then functional.mlp_backward_multi on that forward's saved
state under each pattern of upstream gradient (one network = the single-network entry plnerf_mlp_bwd, bit for bit; two
networks in one call at the end).  Networks whose ReLU units are decisively on or off over the rows (the recipe of the
strict ray-gradient tests: closed-form weights, every unit's bias moved off its range over the rows), so that the
16-bit forward takes the fp64 reference's branches and the comparison is sharp on every row.

Per pattern:
  (a) every gradient tensor within 6e-3 of the fp64 reference's max |g| of that tensor -- the bound tests/test_gpu_modes.py
      states for the dense half-plane backward (G6_GRAD_TOL's coarse figure, and the 6e-3 of its embedded-rows test); the
      reference is fp64 autograd of oracle.nerf_mlp on the same rows' encodings;
  (b) two runs are bit-identical;
  (c) with the saved planes (and ReLU masks) of the zero-gradient rows overwritten by NaN (0xff) the gradients are (b)'s bit
      for bit: the zero rows are not read (a dense backward turns them into NaN gradients: 0 * NaN -- checked once);
  (d) the PLNERF_BWD_COMPACT=0 leg (the switch is read at every call) meets (a) on the same inputs; the largest
      compact-versus-dense difference is printed.
All zero: every tensor exactly 0.
"""
import os

import pytest
import torch

from gpu_support import P, dev, g, make_net
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 6e-3                      # of max |reference| per tensor (tests/test_gpu_modes.py: the dense half-plane backward)
SV_ROW_PAD, W, HV, PE_K, DPE_K = 256, 256, 128, 64, 32      # mlp_layout.h
SHAPES = {421: (421, 1), 2 * 192 + 64: (7, 64)}             # rows: (rays, samples per ray)
BOX = 2.5


def decisive_state_dict(seed, pts, vd, margin=1.5):
    """closed_form_state_dict(seed, True) with every hidden unit's bias moved so that over the rows (pts [R, S, 3], vd [R, 3],
    fp64) the unit is ON everywhere or OFF everywhere (at random), at least 0.05 + a quarter of its range away from zero."""
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
    least = float("inf")
    for i in range(orc.DEPTH):
        z = decide(F.linear(h, sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]), f"pts_linears.{i}.bias")
        least = min(least, float(z.abs().min()))
        h = F.relu(z)
        if i == orc.SKIP_AFTER:
            h = torch.cat([enc_xyz, h], -1)
    feat = F.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
    zv = decide(F.linear(torch.cat([feat, enc_dir], -1), sd["views_linears.0.weight"], sd["views_linears.0.bias"]), "views_linears.0.bias")
    least = min(least, float(zv.abs().min()))
    assert least >= 0.05, least
    # the heads rescaled to a scene-like range, as that recipe does (density ~ N(0.3, 0.06^2), colours of spread 1.5): with the
    # sharpened density head left as it is, g_sigma's path outweighs the colours' by orders of magnitude in every dz plane
    sigma = F.linear(h, sd["alpha_linear.weight"], sd["alpha_linear.bias"])
    rgb = F.linear(F.relu(zv), sd["rgb_linear.weight"], sd["rgb_linear.bias"])
    k_s = 0.06 / float(sigma.std())
    sd["alpha_linear.weight"] *= k_s
    sd["alpha_linear.bias"] = (sd["alpha_linear.bias"] - sigma.mean()) * k_s + 0.3
    k_c = 1.5 / rgb.std(0)
    sd["rgb_linear.weight"] *= k_c[:, None]
    sd["rgb_linear.bias"] = (sd["rgb_linear.bias"] - rgb.mean(0)) * k_c
    return {k: v.float() for k, v in sd.items()}


def patterns(n):
    """name -> bool [n]: which rows carry gradient."""
    gen = torch.Generator().manual_seed(7 + n)
    out = {"all live": torch.ones(n, dtype=torch.bool), "all zero": torch.zeros(n, dtype=torch.bool)}
    for name, k in (("first", 0), ("last", n - 1), ("row 191", 191), ("row 192", 192), ("row 193", 193)):
        m = torch.zeros(n, dtype=torch.bool)
        m[k] = True
        out["one live: " + name] = m
    for k in (31, 32, 33, 63, 64, 65, 191, 192, 193):
        m = torch.zeros(n, dtype=torch.bool)
        m[torch.randperm(n, generator=gen)[:k]] = True
        out[f"{k} live, scattered"] = m
    r = torch.arange(n) % 192
    out["ray pattern 65 live / 126 zero / 1 live"] = (r < 65) | (r == 191)
    out["every other row"] = torch.arange(n) % 2 == 0
    return out


def plane_index(layout, rows, width):
    """Positions (in halves, from the plane's start) of every element of `rows` of a `width`-wide saved plane: row-major, or the
    tiled order of mlp_layout.h (sv_tiled_index)."""
    col = torch.arange(width)[None, :]
    row = rows[:, None]
    if layout == 0:
        return (row * width + col).reshape(-1)
    return ((row >> 5) * (32 * width) + ((((col >> 5) * 2 + ((col >> 4) & 1)) * 2 + ((col >> 2) & 1)) * 32 + (row & 31)) * 8 +
            (((col >> 3) & 1) * 4 + (col & 3))).reshape(-1)


def poisoned(saved, layout, n, zero_rows):
    """A copy of the saved state with every plane element of `zero_rows` NaN and their ReLU mask bytes 0xff."""
    out = saved.clone()
    if zero_rows.numel() == 0:
        return out
    nsv = (n + SV_ROW_PAD - 1) // SV_ROW_PAD * SV_ROW_PAD
    halves = out.view(torch.float16)
    off = 0
    for width, count in ((W, 8), (HV, 1), (PE_K, 1), (DPE_K, 1)):      # h0..h7, hv, pe, dpe: plane-major, rows padded to nsv
        idx = plane_index(layout, zero_rows, width)
        for _ in range(count):
            halves[g(idx + off)] = float("nan")
            off += width * nsv
    assert off == 2272 * nsv
    masks = out.view(torch.uint8)[2272 * 2 * nsv:]
    for p in range(8):
        masks[p * 32 * nsv:(p + 1) * 32 * nsv].view(nsv, 32)[g(zero_rows)] = 0xff
    masks[8 * 32 * nsv:8 * 32 * nsv + 16 * nsv].view(nsv, 16)[g(zero_rows)] = 0xff
    return out


class Forward:
    """One network's training forward at `rows`, kept for many backwards: the MlpFn output (its grad_fn holds the saved state),
    the fp64 reference's output on the same rows, and the decisive weights."""

    def __init__(self, P, Fn, precision, n, seed):
        R, S = SHAPES[n]
        gen = torch.Generator().manual_seed(100 * seed + n)
        pts = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * BOX
        vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
        self.n = n
        sd = decisive_state_dict(seed, pts.double(), vd.double())
        self.net = make_net(P, sd, precision)
        Fn.MLP_TAPE = tape = Fn.MlpTape()
        try:
            self.net.query(g(pts), g(vd))
        finally:
            Fn.MLP_TAPE = None
        (self.out,) = tape.outs
        self.ctx = self.out.grad_fn
        self.saved, self.layout = self.ctx.saved_acts, self.ctx.saved_layout
        named = list(self.net.named_parameters())
        self.names = [next(k for k, q in named if q is p) for p in self.net.param_list()]      # the order of the 24 gradients
        assert len(self.names) == 24 and len(set(self.names)) == 24
        self.sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        emb = torch.cat([orc.positional_encoding(pts.reshape(-1, 3).double(), orc.XYZ_FREQS),
                         orc.positional_encoding(vd.double()[:, None].expand(R, S, 3).reshape(-1, 3), orc.DIR_FREQS)], -1)
        self.raw64 = orc.nerf_mlp(self.sd64, emb)
        self.cot = torch.randn(n, 4, generator=gen)

    def gradient(self, live):
        return (self.cot * live[:, None]).contiguous()      # float32 [n, 4], zero rows exactly (+)0

    def reference(self, g_raw):
        grads = torch.autograd.grad((self.raw64 * g_raw.double()).sum(), [self.sd64[k] for k in self.names], retain_graph=True)
        return dict(zip(self.names, grads))


def backward(Fn, forwards, g_raws, saved=None):
    """mlp_backward_multi on the forwards' saved state (a used-up state is put back first): per network {name: gradient}."""
    for k, f in enumerate(forwards):
        f.ctx.saved_acts = f.saved if saved is None else saved[k]
    grads = Fn.mlp_backward_multi([f.out for f in forwards], [g(x) for x in g_raws])
    torch.cuda.synchronize()
    return [dict(zip(f.names, (t.clone() for t in gr))) for f, gr in zip(forwards, grads)]


def dense(fn):
    """fn() with PLNERF_BWD_COMPACT=0."""
    found = os.environ.get("PLNERF_BWD_COMPACT")
    os.environ["PLNERF_BWD_COMPACT"] = "0"
    try:
        return fn()
    finally:
        if found is None:
            del os.environ["PLNERF_BWD_COMPACT"]
        else:
            os.environ["PLNERF_BWD_COMPACT"] = found


def worst_error(got, ref):
    """max over the tensors of max |got - ref| / max |ref|."""
    worst = 0.0
    for k, r in ref.items():
        scale = float(r.abs().max())
        assert scale > 0.0, k
        err = float((got[k].cpu().double() - r).abs().max()) / scale
        if os.environ.get("PLNERF_TEST_VERBOSE"):
            print(f"    {k}: {err:.2e} of max |ref| {scale:.2e}")
        worst = max(worst, err)
    return worst


def same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def check(Fn, forwards, lives, what):
    """(a)..(d) for one call over `forwards` with the rows `lives` of each carrying gradient."""
    g_raws = [f.gradient(live) for f, live in zip(forwards, lives)]
    first = backward(Fn, forwards, g_raws)
    again = backward(Fn, forwards, g_raws)
    poison = [poisoned(f.saved, f.layout, f.n, (~live).nonzero().reshape(-1)) for f, live in zip(forwards, lives)]
    blind = backward(Fn, forwards, g_raws, poison)
    full = dense(lambda: backward(Fn, forwards, g_raws))
    for f, live, g_raw, a, b, c, d in zip(forwards, lives, g_raws, first, again, blind, full):
        assert all(bool(torch.isfinite(t).all()) for t in a.values()), what
        assert same(a, b), (what, "two runs differ")                                   # (b)
        assert same(a, c), (what, "a zero-gradient row's saved state was read")       # (c)
        if not bool(live.any()):
            for src in (a, d):
                assert all(float(t.abs().max()) == 0.0 for t in src.values()), (what, "all zero")
            print(f"{what} [{f.n} rows, none live]: every gradient exactly 0")
            continue
        ref = f.reference(g_raw)
        e_compact, e_dense = worst_error(a, ref), worst_error(d, ref)
        diff = max(float((a[k] - d[k]).abs().max()) / float(ref[k].abs().max()) for k in a)
        print(f"{what} [{f.n} rows, {int(live.sum())} live]: worst error / max |ref| compact {e_compact:.2e}, dense {e_dense:.2e}; "
              f"compact vs dense {diff:.2e}")
        assert e_compact <= TOL, (what, e_compact)                                      # (a)
        assert e_dense <= TOL, (what, e_dense)                                          # (d)
        assert diff <= TOL, (what, diff)


@pytest.fixture(scope="module")
def Fn(P):
    from plnerf_amd import functional
    return functional


@pytest.fixture(scope="module")
def forwards(P, Fn):
    made = {}

    def get(precision, n, seed=0):
        key = (precision, n, seed)
        if key not in made:
            made[key] = Forward(P, Fn, precision, n, seed)
        return made[key]
    return get


@pytest.mark.parametrize("n", sorted(SHAPES))
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_backward_over_live_rows(Fn, forwards, precision, n):
    f = forwards(precision, n)
    for name, live in patterns(n).items():
        check(Fn, [f], [live], f"{precision}, {name}")


@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_two_networks_in_one_call_one_of_them_all_zero(Fn, forwards, precision):
    a, b = forwards(precision, 421), forwards(precision, 2 * 192 + 64, seed=1)
    pa, pb = patterns(a.n), patterns(b.n)
    check(Fn, [a, b], [pa["all zero"], pb["ray pattern 65 live / 126 zero / 1 live"]], f"{precision}, two networks, first all zero")
    check(Fn, [a, b], [pa["33 live, scattered"], pb["all zero"]], f"{precision}, two networks, second all zero")
    check(Fn, [a, b], [pa["every other row"], pb["all live"]], f"{precision}, two networks")


def test_a_dense_backward_reads_the_zero_rows(Fn, forwards):
    """What (c) rests on: the poison reaches the gradients when the rows ARE read."""
    f = forwards("f16x3", 421)
    live = patterns(f.n)["every other row"]
    poison = poisoned(f.saved, f.layout, f.n, (~live).nonzero().reshape(-1))
    (got,) = dense(lambda: backward(Fn, [f], [f.gradient(live)], [poison]))
    assert any(bool(torch.isnan(t).any()) for t in got.values())
