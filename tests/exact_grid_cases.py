"""The CPU side of tests/test_gpu_exact_grid.py: a network and rows on which the MLP kernels' arithmetic is EXACT, and the
float64 reference they must then equal in every entry (tests/test_exact_grid_host.py checks the conditions without a GPU).

Network (seeded): the compiled trunk's 24 tensors (oracle.param_shapes()); every row of a hidden weight (trunk, feature and
view layer) has HIDDEN_NNZ = 3 nonzeros, each +-1, at random columns; alpha_linear and rgb_linear have HEAD_NNZ = 16 per
row; biases are in {-1, 0, 1}.  (With 4 nonzeros per row the activations pass 255.)
Rows: `embedded` [n, 63 + 27] integers in [-4, 4] (the caller-supplied encoding: sin / cos cannot be exact); `g_raw` [n, 4]
integers in [-2, 2]; about 30 % of the rows have g_raw exactly zero (the backward's live-row compaction skips them), the last
row is always live, and from n = 192 on rows 64..127 are a whole dead 64-row tile and row 191 is the only live row of rows
128..191.
Reference: orc.nerf_mlp and autograd in float64.  The post-ReLU activations and `feat` keep their gradients; a
pre-activation's gradient is dz = dh * (h > 0), which is what autograd's ReLU applies (pre-activation 0 included: no
gradient), so the module sees what the kernels store: the saved activations and the pre-activation gradient planes.

What build() asserts (a seed that misses one fails loudly):
  a. 8-bit forward values: every input, weight, bias, hidden activation, feat, view-layer activation, and the composed view
     layer's weight W_v[:, :256] W_f and bias W_v[:, :256] b_f + b_v, is an integer with |v| <= 255 -- bf16's 8 significant
     bits, so one fixture serves all five modes.
  b. the pre-activation gradients fit the half planes: every dz and d feat is an integer, and with the launch scale 2^s of
     include/plnerf_hip.h ("Backward of modes 1-4": max |g_raw| = m 2^e, 0.5 <= m < 1, s = 4 - e) |dz| 2^s <= 2048: every
     scaled entry is an integer no wider than the IEEE half's 11 bits.
  c. exact sums in any order: for every forward contraction, every step of the gradient chain, every gradient entry and
     g_embedded, the sum of the absolute values of its terms is below 2^24, so every partial sum in any order, split or
     not, is an integer that fp32 holds; every reference tensor equals its own float32 cast.
  d. nothing degenerate: every ReLU layer is live on 25-75 % of its units; from n = 33 on each of the 24 gradient tensors
     and g_embedded has at least 15 % nonzero entries, at n = 1000 at least 25 %.
"""
import functools

import numpy as np
import torch

from oracle import plnerf_oracle as orc

ROWS = (1, 33, 64, 65, 193, 257, 1000)      # one row; either side of the 32-, 64-, 192- and 256-row tiles; ragged against all
SEED, SECOND_SEED = 1, 2
TWO_JOBS = ((193, SEED), (65, SECOND_SEED))      # plnerf_mlp_bwd_multi's two jobs
CASES = tuple((n, SEED) for n in ROWS) + (TWO_JOBS[1],)      # every (rows, seed) the GPU test builds
HIDDEN_NNZ, HEAD_NNZ = 3, 16
INPUT_MAX, COTANGENT_MAX, DEAD_SHARE = 4, 2, 0.3
XC, DC = orc.XYZ_CH, orc.DIR_CH
RELU_LAYERS = [f"pts_linears.{i}" for i in range(orc.DEPTH)] + ["views_linears.0"]
EXACT = 2.0 ** 24


def launch_shift(g_absmax):
    """s of the 16-bit backward's launch scale 2^s for max |g_raw| = m 2^e (0.5 <= m < 1): s = 4 - e, the maximum -> [8, 16)."""
    m, e = np.frexp(np.float32(g_absmax))
    assert 0.5 <= m < 1.0, g_absmax
    return 4 - int(e)


@functools.lru_cache(maxsize=None)
def network(seed):
    """{name: float32 tensor} in state_dict order."""
    rng = np.random.default_rng([seed, 11])
    sd = {}
    for name, shape in orc.param_shapes():
        if len(shape) == 1:
            w = rng.integers(-1, 2, shape)
        else:
            nnz = HEAD_NNZ if name.startswith(("alpha_linear", "rgb_linear")) else HIDDEN_NNZ
            w = np.zeros(shape, np.int64)
            for r in range(shape[0]):
                w[r, rng.choice(shape[1], nnz, replace=False)] = rng.choice([-1, 1], nnz)
        sd[name] = torch.from_numpy(w.astype(np.float32))
    return sd


def rows(n, seed):
    """(embedded [n, 90], g_raw [n, 4]) float32 integers."""
    rng = np.random.default_rng([seed, n, 13])
    emb = rng.integers(-INPUT_MAX, INPUT_MAX + 1, (n, XC + DC))
    g = rng.integers(-COTANGENT_MAX, COTANGENT_MAX + 1, (n, 4))
    empty = ~g.any(-1)      # a live row is not zero: one entry of it becomes 1 or 2
    g[empty, np.arange(n)[empty] % 4] = 1 + np.arange(n)[empty] % 2
    dead = rng.random(n) < DEAD_SHARE
    if n >= 192:
        dead[64:191], dead[191] = True, False
    dead[n - 1] = False
    g[dead] = 0
    if g[:, 3].sum() == 0:      # alpha_linear.bias has one entry, the sum of this column: the last row moves it off zero
        v = g[n - 1, 3]
        g[n - 1, 3] = next(u for u in (v + 1, v - 1) if abs(u) <= COTANGENT_MAX and (u or g[n - 1, :3].any()))
    return emb.astype(np.float32), g.astype(np.float32)


def _integers(name, t, bound):
    a = np.asarray(t, np.float64)
    assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= bound, (name, "not an integer within", bound, float(np.abs(a).max()))
    return float(np.abs(a).max())


class Case:
    """One (rows, seed): the inputs, the float64 reference as float32 arrays (raw, grads in state_dict order, g_embedded),
    and the measured margins (`stats`)."""


@functools.lru_cache(maxsize=None)
def build(n, seed):
    c = Case()
    c.n, c.seed, c.sd = n, seed, network(seed)
    c.embedded, c.g_raw = rows(n, seed)
    c.names = [name for name, _ in orc.param_shapes()]
    live_rows = c.g_raw.any(-1)
    assert live_rows[-1] and (n < 192 or (not live_rows[64:191].any() and live_rows[191]))
    c.shift = launch_shift(np.abs(c.g_raw).max())

    sd64 = {k: v.double().requires_grad_(True) for k, v in c.sd.items()}
    emb = torch.from_numpy(c.embedded).double().requires_grad_(True)
    raw, hidden = orc.nerf_mlp(sd64, emb, return_hidden=True)
    for h in hidden:
        h.retain_grad()
    (raw * torch.from_numpy(c.g_raw).double()).sum().backward()
    act = [h.detach().numpy() for h in hidden]      # h0..h7, feat, hv
    feat, hv = act[8], act[9]
    dz = [(h.grad * (h > 0)).numpy() for h in hidden[:8]] + [hidden[8].grad.numpy(), (hidden[9].grad * (hidden[9] > 0)).numpy()]
    W = {k: v.detach().numpy() for k, v in sd64.items()}
    x, d, g = c.embedded[:, :XC].astype(np.float64), c.embedded[:, XC:].astype(np.float64), c.g_raw.astype(np.float64)
    w_view, b_view = W["views_linears.0.weight"], W["views_linears.0.bias"]
    w_comp = w_view[:, :orc.WIDTH] @ W["feature_linear.weight"]
    b_comp = w_view[:, :orc.WIDTH] @ W["feature_linear.bias"] + b_view

    # a. 8-bit forward values
    stats = c.stats = {}
    for name, v in W.items():
        _integers(name, v, 1)
    _integers("embedded", c.embedded, INPUT_MAX)
    _integers("g_raw", g, COTANGENT_MAX)
    stats["max activation"] = max(_integers(f"activation {i}", a, 255) for i, a in enumerate(act))
    stats["max composed view layer"] = max(_integers("composed view weight", w_comp, 255), _integers("composed view bias", b_comp, 255))
    _integers("raw", raw.detach().numpy(), EXACT)

    # b. the pre-activation gradients fit the half planes
    stats["max |dz|"] = max(_integers(f"dz {i}", a, 2048 / 2.0 ** c.shift) for i, a in enumerate(dz))

    # c. exact sums in any order: sum |terms| of every contraction
    layer_in = [x] + act[:4] + [np.concatenate([x, act[4]], -1)] + act[5:7]      # what trunk layer i reads
    sums = {}
    for i in range(orc.DEPTH):
        w, b = W[f"pts_linears.{i}.weight"], W[f"pts_linears.{i}.bias"]
        sums[f"forward {i}"] = np.abs(layer_in[i]) @ np.abs(w).T + np.abs(b)
        sums[f"pts_linears.{i}.weight"] = np.abs(dz[i]).T @ np.abs(layer_in[i])
        sums[f"pts_linears.{i}.bias"] = np.abs(dz[i]).sum(0)
        sums[f"chain {i}"] = np.abs(dz[i]) @ np.abs(w)
    h7, view_in = act[7], np.concatenate([feat, d], -1)
    sums["forward feat"] = np.abs(h7) @ np.abs(W["feature_linear.weight"]).T + np.abs(W["feature_linear.bias"])
    sums["forward view"] = np.abs(view_in) @ np.abs(w_view).T + np.abs(b_view)
    sums["forward composed view"] = np.abs(h7) @ np.abs(w_comp).T + np.abs(d) @ np.abs(w_view[:, orc.WIDTH:]).T + np.abs(b_comp)
    sums["raw rgb"] = np.abs(hv) @ np.abs(W["rgb_linear.weight"]).T + np.abs(W["rgb_linear.bias"])
    sums["raw sigma"] = np.abs(h7) @ np.abs(W["alpha_linear.weight"]).T + np.abs(W["alpha_linear.bias"])
    sums["views_linears.0.weight"] = np.abs(dz[9]).T @ np.abs(view_in)
    sums["views_linears.0.bias"] = np.abs(dz[9]).sum(0)
    sums["feature_linear.weight"] = np.abs(dz[8]).T @ np.abs(h7)
    sums["feature_linear.bias"] = np.abs(dz[8]).sum(0)
    sums["alpha_linear.weight"] = np.abs(g[:, 3:]).T @ np.abs(h7)
    sums["alpha_linear.bias"] = np.abs(g[:, 3:]).sum(0)
    sums["rgb_linear.weight"] = np.abs(g[:, :3]).T @ np.abs(hv)
    sums["rgb_linear.bias"] = np.abs(g[:, :3]).sum(0)
    sums["chain rgb"] = np.abs(g[:, :3]) @ np.abs(W["rgb_linear.weight"])
    sums["chain view"] = np.abs(dz[9]) @ np.abs(w_view)
    sums["chain head"] = (np.abs(dz[8]) @ np.abs(W["feature_linear.weight"]) + np.abs(dz[9]) @ np.abs(w_comp)
                          + np.abs(g[:, 3:]) @ np.abs(W["alpha_linear.weight"]))      # d h7, by the feature layer or the composed one
    sums["g_embedded xyz"] = (np.abs(dz[0]) @ np.abs(W["pts_linears.0.weight"])
                              + np.abs(dz[5]) @ np.abs(W["pts_linears.5.weight"][:, :XC]))
    sums["g_embedded dir"] = np.abs(dz[9]) @ np.abs(w_view[:, orc.WIDTH:])
    assert set(c.names) <= set(sums)
    for what, s in sums.items():
        assert s.max() < EXACT, (what, "sum of |terms|", float(s.max()))
    stats["max sum |terms|"] = max(float(s.max()) for s in sums.values())
    stats["max sum |terms| of pts_linears.3.weight"] = float(sums["pts_linears.3.weight"].max())

    def f32(name, t):
        a = t.detach().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), (name, "is not its own float32 cast")
        return a.astype(np.float32)
    c.raw = f32("raw", raw)
    c.grads = [f32(name, sd64[name].grad) for name in c.names]
    c.g_embedded = f32("g_embedded", emb.grad)

    # d. nothing degenerate
    shares = [float((a > 0).mean()) for a in act[:8] + [hv]]
    stats["live share per ReLU layer"] = (min(shares), max(shares))
    for name, share in zip(RELU_LAYERS, shares):
        assert 0.25 <= share <= 0.75, (name, "live on", share)
    nonzero = {name: float((a != 0).mean()) for name, a in zip(c.names + ["g_embedded"], c.grads + [c.g_embedded])}
    stats["smallest nonzero share"] = min(nonzero.values())
    stats["zero rows"] = float(1.0 - live_rows.mean())
    floor = 0.25 if n == 1000 else 0.15 if n >= 33 else 0.0
    for name, share in nonzero.items():
        assert share >= floor and share > 0, (name, "nonzero share", share, "at", n, "rows")
    for a in [c.embedded, c.g_raw, c.raw, c.g_embedded] + c.grads:
        a.setflags(write=False)
    return c
