"""What the encoding tests (tests/test_pe_probe_host.py on the CPU, tests/test_gpu_encoding.py on the GPU) share, each written
once: the float64 yardstick of the positional encoding on the SAME fp32 argument the kernels form, a one-hot network that
hands chosen encoding channels through to its four outputs without arithmetic error of its own, the sweep of coordinates
(magnitude ladder, multiples of pi/2, rint ties, straddlers of every branch limit) in its arrangements, the predicates of the
kernels' two arithmetic paths, and the closed-form weight gradients of the one-hot network.

numpy and torch on the CPU only.  A plain module, so pytest does not rewrite its asserts: every assert carries its message."""
import functools
import math
import types

import numpy as np
import torch

from oracle import plnerf_oracle as orc

F32 = np.float32
XYZ_BANDS, DIR_BANDS = orc.XYZ_FREQS, orc.DIR_FREQS      # the bands every kernel EVALUATES, whatever the network's widths
FAST_LIMIT = 2.0 ** 22            # pe_sincos.h: PE_FAST_LIMIT
NEAR_BOUND = 1.2e-7               # pe_sincos.h's own figure for the shared reduction (2 ulp of one)
MAX_ABS_F16, MAX_ABS_F32 = 6.0e4, 2.0 ** 30      # f16-element modes (the identity channel is a half operand) | the others
CONFIGS = {"nvs": (63, 27, 1.0), "depth": (57, 3, math.pi)}      # input_ch | input_ch_views | the encoder's input scale
MUTE_BELOW, MUTE_CAP = 1e-6, 0.02


# ----------------------------------------------------------------------------- the yardstick
def band_arguments(x32, n_freqs, scale):
    """fl(fl(x * s) * 2^k) in fp32, the reference's association: [..., n_freqs, 3] float32 (the second product is exact)."""
    x32 = np.asarray(x32, dtype=F32)
    xs = x32 * F32(scale)
    assert xs.dtype == F32, "the scaled coordinate must be an fp32 product"
    return xs[..., None, :] * (F32(2.0) ** np.arange(n_freqs, dtype=F32))[:, None]


def reference_encoding(x32, n_freqs, scale):
    """gamma(x) = [x | sin, cos of fl(fl(x s) 2^k), k < n_freqs] with the sines / cosines of that fp32 argument taken in
    float64: [..., 3 + 6 n_freqs] float64, channels in the reference's order (per band: sin xyz, cos xyz)."""
    x32 = np.asarray(x32, dtype=F32)
    arg = band_arguments(x32, n_freqs, scale).astype(np.float64)
    bands = np.concatenate([np.sin(arg), np.cos(arg)], -1)      # [..., n_freqs, 6]
    return np.concatenate([x32.astype(np.float64), bands.reshape(*x32.shape[:-1], 6 * n_freqs)], -1)


def channel(band, coord, cos=False):
    """Column of sin / cos(coordinate `coord` at band `band`) in an encoding row."""
    return 3 + 6 * band + (3 if cos else 0) + coord


def far_elements(x32, n_bands, scale):
    """The exact-fp32 kernel's per-element predicate, as encoding columns: [..., 3 + 6 n_bands] bool, True where the element
    is past the shared reduction (|argument| >= 2^22: library sincosf).  The identity columns are False."""
    far = np.abs(band_arguments(x32, n_bands, scale)) >= F32(FAST_LIMIT)
    far6 = np.concatenate([far, far], -1).reshape(*far.shape[:-2], 6 * n_bands)
    return np.concatenate([np.zeros(far.shape[:-2] + (3,), bool), far6], -1)


def far_halves(x32, n_bands, scale):
    """The register-resident / ping-pong kernels' predicate per lane half: [..., 2] bool, half g holds bands
    g n/2 .. (g + 1) n/2 - 1 and is far when max |coordinate * s| * 2^(its top band) >= 2^22 -- then ALL its bands, small
    coordinates included, go through sincosf."""
    top = np.abs(np.asarray(x32, dtype=F32) * F32(scale)).max(-1)
    return np.stack([top * F32(2.0 ** (n_bands // 2 - 1)) >= F32(FAST_LIMIT), top * F32(2.0 ** (n_bands - 1)) >= F32(FAST_LIMIT)], -1)


def far_rows(x32, n_bands, scale):
    """Rows with anything past the shared reduction in ANY kernel (the top band's predicate: the first to go far)."""
    return far_halves(x32, n_bands, scale)[..., 1]


# ----------------------------------------------------------------------------- the one-hot network
def probe_outputs(n_xyz, n_dirs):
    """Output columns (of raw = [r, g, b, sigma]) that carry probe_state_dict's chosen channels: xyz first, then dirs."""
    assert n_xyz <= 4 and max(n_xyz - 1, 0) + n_dirs <= 3, ("a forward reads up to 4 xyz or 3 direction channels", n_xyz, n_dirs)
    return ([3] + list(range(n_xyz - 1)) if n_xyz else []) + list(range(max(n_xyz - 1, 0), max(n_xyz - 1, 0) + n_dirs))


def probe_state_dict(xyz=(), dirs=(), xyz_ch=63, dir_ch=27):
    """A network whose four outputs ARE chosen encoding channels.  xyz channel number i enters the trunk as the +/- pair of
    hidden units 2 i, 2 i + 1 (weights +1 / -1), rides layers 1..7 on identities (layer 5's sit behind the re-injected
    encoding columns, which are zero) and leaves as relu(v) - relu(-v) = v: the first through alpha_linear, the others
    through feature_linear, the view layer (units 2 j, 2 j + 1 of colour slot j) and rgb_linear.  Direction channels enter
    the view layer's last columns as +/- pairs of the colour slots behind them.  Every other product has a zero factor and
    every bias is zero, so the read-out is exact in fp32 for finite inputs (and in the 16-bit modes up to the one operand
    rounding of the value itself: W_vf W_f is a product of one-hot matrices)."""
    probe_outputs(len(xyz), len(dirs))
    assert all(0 <= c < xyz_ch for c in xyz) and all(0 <= c < dir_ch for c in dirs), (xyz, dirs, xyz_ch, dir_ch)
    sd = {name: torch.zeros(shape) for name, shape in orc.param_shapes_depth((xyz_ch - 3) // 6, (dir_ch - 3) // 6)}
    W = orc.WIDTH
    for i, c in enumerate(xyz):
        for u, sign in ((2 * i, 1.0), (2 * i + 1, -1.0)):
            sd["pts_linears.0.weight"][u, c] = sign
            for layer in range(1, orc.DEPTH):
                sd[f"pts_linears.{layer}.weight"][u, u + (xyz_ch if layer == orc.SKIP_AFTER + 1 else 0)] = 1.0
            if i == 0:
                sd["alpha_linear.weight"][0, u] = sign
            else:
                j = i - 1
                hv = 2 * j + (u & 1)
                sd["feature_linear.weight"][u, u] = 1.0
                sd["views_linears.0.weight"][hv, u] = 1.0
                sd["rgb_linear.weight"][j, hv] = sign
    for n, c in enumerate(dirs):
        j = max(len(xyz) - 1, 0) + n
        for hv, sign in ((2 * j, 1.0), (2 * j + 1, -1.0)):
            sd["views_linears.0.weight"][hv, W + c] = sign
            sd["rgb_linear.weight"][j, hv] = sign
    return sd


def channel_groups(channels, size):
    """`channels` in groups of at most `size`: one forward of the one-hot network each."""
    channels = list(channels)
    return [tuple(channels[i:i + size]) for i in range(0, len(channels), size)]


# ----------------------------------------------------------------------------- the sweep
def _step(v, k):
    """The float32 k ulps above (k < 0: below) the positive float32 v."""
    return (np.asarray(v, dtype=F32).view(np.int32) + np.int32(k)).view(F32)


def limits(n_bands, scale, max_abs):
    """The coordinate magnitudes at which some kernel changes path, as (band, fl32(2^(22 - band) / s)) within max_abs:
    2^(22 - f) / s is the exact-fp32 kernel's per-element predicate of band f, and bands n/2 - 1 and n - 1 are the register-
    resident and ping-pong kernels' two lane halves (xyz: 2^18 / s and 2^13 / s; directions: 2^21 / s and 2^19 / s)."""
    s = float(F32(scale))
    return [(f, F32(2.0 ** (22 - f) / s)) for f in range(n_bands) if 2.0 ** (22 - f) / s * (1 + 2.0 ** -20) <= max_abs]


def _leads(max_abs, scale, n_bands, rng, full):
    """Magnitudes with a story, signed: (the values, how many trailing ones are limit straddlers -- those come three times,
    once per coordinate)."""
    s = float(F32(scale))
    out = []
    top = int(math.floor(math.log2(max_abs)))
    for e in range(-40 if full else 1, top + 1):      # the ladder: each rung exactly and twice inside the octave
        for m in (1.0, *rng.uniform(1.0, 2.0, 2)):
            out.append(min(2.0 ** e * m, max_abs))
    out.append(max_abs)
    ladder = np.asarray(out, dtype=F32)
    vals = [ladder, -ladder]
    if full:
        vals.append(np.asarray([0.0, -0.0, 2.0 ** -149, -2.0 ** -130, float(_step(F32(2.0 ** -126), -1)), 2.0 ** -126, 1.0, -1.0], dtype=F32))
    # nearest floats to k pi / (2 s) and their two neighbours, k log-spaced up to the limit
    kmax = max_abs * s * 2.0 / math.pi
    ks = np.unique(np.floor(np.logspace(0.0, math.log10(kmax), 110 if full else 40)).astype(np.int64))
    near_k = (ks * (math.pi / (2.0 * s))).astype(F32)
    near_k = np.concatenate([_step(near_k, -1), near_k, _step(near_k, 1)])
    near_k = near_k[np.abs(near_k) <= max_abs]
    vals.append(near_k * np.where(np.arange(near_k.size) % 2 == 0, 1, -1).astype(F32))
    # rint ties of the shared reduction: x s 2/pi 2^f = n + 1/2 (on the fast path: the argument stays below 2^22)
    ties = []
    for f in range(n_bands):
        nmax = min(FAST_LIMIT * 2.0 / math.pi, max_abs * s * 2.0 ** f * 2.0 / math.pi) - 1.0
        for n in np.unique(np.floor(np.logspace(0.0, math.log10(nmax), 12)).astype(np.int64)):
            ties.append((n + 0.5) * math.pi / (2.0 * s * 2.0 ** f))
    ties = np.asarray(ties, dtype=F32)
    vals.append(ties * np.where(np.arange(ties.size) % 2 == 0, -1, 1).astype(F32))
    # every limit: the 24 floats below it, the value itself and the 23 above
    strad = []
    for _, lim in limits(n_bands, scale, max_abs):
        v = np.asarray([_step(lim, k) for k in range(-24, 24)], dtype=F32)
        strad.append(v * np.where(np.arange(v.size) % 2 == 0, 1, -1).astype(F32))
    strad = np.concatenate(strad) if strad else np.zeros(0, F32)
    body = np.concatenate(vals)
    return np.concatenate([body, strad, strad, strad]).astype(F32), 3 * strad.size


def _rows_of(leads, n_strad, rng):
    """One lead per row, in coordinate (row mod 3) (the straddlers' three copies take one coordinate each), the two other
    coordinates small: different rungs of 2^-10 .. 2^-1, random mantissa and sign."""
    n = leads.size
    rungs = np.argsort(rng.random((n, 10)), axis=1)[:, :3] - 10      # three distinct exponents per row
    small = (2.0 ** rungs * rng.uniform(1.0, 2.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(F32)
    where = np.arange(n) % 3
    if n_strad:
        where[n - n_strad:] = np.repeat(np.arange(3), n_strad // 3)
    small[np.arange(n), where] = leads
    return small


@functools.lru_cache(maxsize=None)
def sweep(max_abs, scale, seed=0):
    """A few thousand rows of (pts, per-ray dirs), all finite, |coordinate| <= max_abs, for the encoder input scale `scale`:
    .pts / .dirs [N, 3] float32 in building order; .perm[name] for name in ARRANGEMENTS with arrangement = rows[perm] (so
    out_in_building_order[perm] = out_of_arrangement); .far [N]: rows with anything past the shared reduction in any kernel
    (position or direction); .pts7 / .dirs7: the interleaved rows as rays of seven samples ([7 R, 3] | [R, 3]).  N mod 32 is
    13: the last wave is ragged.  Cached: treat every array as read-only."""
    rng = np.random.default_rng(seed)
    leads, n_strad = _leads(max_abs, scale, XYZ_BANDS, rng, True)
    pts = _rows_of(leads, n_strad, rng)
    far_x = far_rows(pts, XYZ_BANDS, scale)
    # directions: unit vectors (the six axes among them); a second set scaled up to max_abs, most of it on rows whose
    # position is far already, a hundred on near rows
    d_leads, d_strad = _leads(max_abs, scale, DIR_BANDS, rng, False)
    big = _rows_of(d_leads, d_strad, rng)
    big = big[rng.permutation(big.shape[0])]
    n = pts.shape[0]
    near_idx, far_idx = np.flatnonzero(~far_x), np.flatnonzero(far_x)
    assert big.shape[0] - 100 <= far_idx.size, ("more scaled-up directions than far rows to carry them", big.shape[0], far_idx.size)
    # fill with near rows until the arrangements below have what they need: 64 waves of 31 near rows + 1 far row
    n_fill = max(0, 2200 - near_idx.size)
    fill = (2.0 ** rng.uniform(-6.0, math.log2(0.999 * 2.0 ** 13 / float(F32(scale))), n_fill) * rng.choice([-1.0, 1.0], n_fill)).astype(F32)
    n_fill += (13 - (n + n_fill)) % 32
    fill = np.concatenate([fill, rng.uniform(-3.0, 3.0, n_fill - fill.size).astype(F32)])
    pts = np.concatenate([pts, _rows_of(fill, 0, rng)])
    N = pts.shape[0]
    assert N % 32 == 13, N
    unit = rng.standard_normal((N, 3))
    dirs = (unit / np.linalg.norm(unit, axis=-1, keepdims=True)).astype(F32)
    picks = near_idx[np.linspace(0, near_idx.size - 1, 100).astype(np.int64)]
    dirs[picks] = big[:100]
    dirs[far_idx[:big.shape[0] - 100]] = big[100:]
    dirs[np.setdiff1d(near_idx, picks)[:6]] = np.asarray([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F32)
    assert np.isfinite(pts).all() and np.isfinite(dirs).all() and np.abs(pts).max() <= max_abs and np.abs(dirs).max() <= max_abs
    far = far_rows(pts, XYZ_BANDS, scale) | far_rows(dirs, DIR_BANDS, scale)
    fi, ni = np.flatnonzero(far), np.flatnonzero(~far)
    perm = {}
    # sorted by magnitude, near rows first: whole 128-row tiles are all-near or all-far
    perm["sorted"] = np.lexsort((np.abs(pts).max(-1), far))
    # interleaved: the far rows evenly spread, so every wave mixes far and near rows
    slots = np.floor(np.arange(fi.size) * (N / fi.size)).astype(np.int64)
    inter = np.full(N, -1, np.int64)
    inter[slots] = fi
    inter[inter < 0] = ni
    perm["interleaved"] = inter
    # single far row: waves of 31 near rows and one far row, at row 0, 15, 16, 31 of a tile's first .. fourth wave; what is
    # left over follows, near rows first
    n_w = min(ni.size // 31, fi.size)
    waves = []
    for w in range(n_w):
        at = (0, 15, 16, 31)[w % 4]
        waves.append(np.insert(ni[31 * w:31 * w + 31], at, fi[w]))
    perm["single_far"] = np.concatenate(waves + [ni[31 * n_w:], fi[n_w:]])
    for name, p in perm.items():
        assert np.array_equal(np.sort(p), np.arange(N)), f"{name} is not a permutation"
    R7 = N // 7
    if (7 * R7) % 32 == 0:
        R7 -= 1
    return types.SimpleNamespace(pts=pts, dirs=dirs, perm=perm, far=far, n_single=n_w, max_abs=max_abs, scale=scale,
                                 pts7=pts[inter][:7 * R7].copy(), dirs7=dirs[inter][:7 * R7:7].copy())


ARRANGEMENTS = ("sorted", "interleaved", "single_far")


def fast_path_records(sw):
    """Every (scaled coordinate fl(x s), band) pair of the sweep that the shared reduction serves in the exact-fp32 kernel
    (|argument| < 2^22), positions and directions: a structured array of (float32 xs, int32 band)."""
    rec = []
    for x, nb in ((sw.pts, XYZ_BANDS), (sw.dirs, DIR_BANDS)):
        xs = x * F32(sw.scale)
        arg = band_arguments(x, nb, sw.scale)
        for f in range(nb):
            keep = np.abs(arg[:, f, :]) < F32(FAST_LIMIT)
            v = xs[keep]
            r = np.zeros(v.size, dtype=[("xs", "<f4"), ("band", "<i4")])
            r["xs"], r["band"] = v, f
            rec.append(r)
    return np.concatenate(rec)


# ----------------------------------------------------------------------------- the one-hot network's weight gradients
# The channels the weight-gradient test routes, from low bands so that few rows are muted (cosines for the positions: a
# small coordinate's sine is small, its cosine is one): cos(band 0, x) -> sigma, cos(band 1, y) -> r; directions: NVS
# sin(band 0, z) -> g, cos(band 1, x) -> b; depth variant (identity only) x -> g, y -> b
WGRAD_ROUTES = {"nvs": ((channel(0, 0, True), channel(1, 1, True)), (channel(0, 2), channel(1, 0, True))),
                "depth": ((channel(0, 0, True), channel(1, 1, True)), (0, 1))}


def muted_rows(enc_xyz, enc_dir, xyz, dirs):
    """Rows whose cotangent is zeroed: a routed channel has 0 < |e| < 1e-6 in the reference, so the side of its pair of ReLUs
    is not determined by the reference alone (e == 0 is: both units are off)."""
    e = np.concatenate([enc_xyz[:, list(xyz)], enc_dir[:, list(dirs)]], -1)
    return ((np.abs(e) > 0) & (np.abs(e) < MUTE_BELOW)).any(-1)


def probe_wgrad_reference(enc_xyz, enc_dir, xyz, dirs, g_raw):
    """The one-hot network's weight gradients that are sums over ONE encoding channel per column, in closed form and float64.
    With e the routed channel and g the cotangent of the output it reaches, the + unit's pre-activation gradient is
    g [e > 0], the - unit's -g [e < 0], the same at every layer of the pair's path, so
        dW[+unit, :] = sum_r g_r [e_r > 0] enc(r, :),      dW[-unit, :] = sum_r -g_r [e_r < 0] enc(r, :).
    Returns {name: (rows, column slice, reference [rows, columns], sum of the terms' magnitudes)} for pts_linears.0.weight,
    the first columns of pts_linears.5.weight and the last columns of views_linears.0.weight."""
    cols = probe_outputs(len(xyz), len(dirs))
    g = np.asarray(g_raw, dtype=np.float64)

    def pair(e, gc):
        return np.stack([gc * (e > 0), -gc * (e < 0)], -1)      # [N, 2]: dz of the + and the - unit
    trunk = np.concatenate([pair(enc_xyz[:, c], g[:, cols[i]]) for i, c in enumerate(xyz)], -1)             # units 0 .. 2 n_xyz - 1
    view = [pair(enc_xyz[:, c], g[:, cols[i]]) for i, c in enumerate(xyz) if i >= 1]
    view += [pair(enc_dir[:, c], g[:, cols[len(xyz) + n]]) for n, c in enumerate(dirs)]
    view = np.concatenate(view, -1)                                                                          # view units 0 .. 2 slots - 1
    xc, dc = enc_xyz.shape[1], enc_dir.shape[1]
    t_ref, t_mag = trunk.T @ enc_xyz, np.abs(trunk).T @ np.abs(enc_xyz)
    v_ref, v_mag = view.T @ enc_dir, np.abs(view).T @ np.abs(enc_dir)
    return {"pts_linears.0.weight": (trunk.shape[1], slice(0, xc), t_ref, t_mag),
            f"pts_linears.{orc.SKIP_AFTER + 1}.weight": (trunk.shape[1], slice(0, xc), t_ref, t_mag),
            "views_linears.0.weight": (view.shape[1], slice(orc.WIDTH, orc.WIDTH + dc), v_ref, v_mag)}
