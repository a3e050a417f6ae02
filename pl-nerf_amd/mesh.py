"""Mesh extraction: the reference's nerf_extract_mesh.py (:531-593, :1087-1106) on the device, without PyMCubes or trimesh.

    from plnerf_amd.mesh import extract_geometry, keep_components, write_ply
    vertices, triangles = extract_geometry(min_xyz, max_xyz, 512, 25, render_kwargs["network_query_fn"],
                                           render_kwargs["network_fine"])
    triangles = triangles[keep_components(triangles, min_len=10000)]
    write_ply("mesh.ply", vertices, triangles)

`extract_fields` is ONE library call (plnerf_density_grid, include/experimental/plnerf_hip_mesh.h) where `model` is a network
that entry serves -- what anyview._route() admits: the compiled trunk with the in-kernel encoding, or a shape outside it under
the standard Embedder pair; NVS networks only (no input scale, no density activation) -- and the reference's loop over 64^3
blocks through `query_func` otherwise.  `marching_cubes` is plnerf_mc_count + plnerf_mc_emit on the device field; there is no
CPU fallback.

CONVENTIONS.  A lattice point is inside when f >= iso (so NaN is outside); vertices are ordered by owning lattice point, then
axis; triangles by cell, then table order; normals point towards decreasing field.  These are this library's, stated in the
header.  Neither PyMCubes nor trimesh was at hand when this was written: the function signatures, the index-coordinate
vertices, and "components of edge-adjacent faces with at least min_len faces" are matched from their written descriptions
only, and nothing is claimed about PyMCubes' vertex / triangle order, orientation, or its treatment of f == iso.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import anyview
from .render import MAX_ROWS_PER_LAUNCH

BLOCK = 64      # extract_fields' block edge (nerf_extract_mesh.py:532)


# ---- the density lattice ---------------------------------------------------------------------------------------------------
def _linspaces(bound_min, bound_max, resolution):
    """The reference's three tables, by its own expression (on the default device, as there)."""
    return [torch.linspace(bound_min[a], bound_max[a], resolution) for a in range(3)]


def _served_route(query_func, model):
    """The slot route plnerf_density_grid would run `model` on, or None (the block loop remains)."""
    from .nerf import NeRF
    emb = getattr(query_func, "embedders", None)      # (create_nerf's query function says what it encodes with)
    if emb is None or not isinstance(model, NeRF) or not torch.cuda.is_available():
        return None
    return anyview._route(model, emb)[0]


def _fill_slot(slot, model, route, device, keep):
    """One plnerf_anyview_net for `model`, as AnyViewRenderer._bind_networks fills it; keep: what the slot points at.
    Returns (the status word tensor or None, the network's precision code, input_ch, input_ch_views)."""
    from . import generic
    slot.route = route
    if route == L.ANYVIEW_FUSED:
        code = L.PRECISION[model.precision]
        packed = torch.zeros(L.lib().plnerf_mlp_packed_bytes(code) // 4, device=device, dtype=torch.float32)
        live = [p.detach() for p in model.param_list()]
        for k, p in enumerate(live):
            slot.fused.params[k] = L.dptr(p, f"params[{k}]").value
        slot.fused.packed = packed.data_ptr()
        keep += [packed, live]
        off = L.lib().plnerf_mlp_status_offset(code) // 4
        return packed.view(torch.int32)[off:off + 1], code, model.input_ch, model.input_ch_views
    live = [t for fc in generic._layers(model) for t in (fc.weight, fc.bias)]
    fp32, table = generic._param_table(live)
    shape = generic._describe(model, torch.empty(0, model.input_ch + model.view_ch, device=device))[0]
    ctypes.memmove(ctypes.byref(slot.shape), ctypes.byref(shape), ctypes.sizeof(shape))
    slot.params = ctypes.cast(table, ctypes.c_void_p).value
    keep += [fp32, table]
    status = None
    if route == L.ANYVIEW_CHAIN16:
        slot.precision = L.PRECISION[model.precision]
        status = model.status_word()
        slot.status = status.data_ptr()
    return status, 0, 0, 0


def density_grid(model, route, xs, ys, zs, max_rows=MAX_ROWS_PER_LAUNCH, stats=True):
    """plnerf_density_grid: (field [res, res, res] fp32 on the device, stats [4] fp64 on the device or None) of `model` on the
    lattice xs x ys x zs (three [res] tables).  Raises FloatingPointError when a 16-bit network left its range."""
    device = next(model.parameters()).device
    res = int(xs.numel())
    tables = [t.detach().to(device=device, dtype=torch.float32).contiguous() for t in (xs, ys, zs)]
    keep = []
    slot = L.AnyViewNet()
    status, code, in_ch, view_ch = _fill_slot(slot, model, route, device, keep)
    lib = L.lib()
    nbytes = lib.plnerf_density_grid_workspace_bytes(ctypes.byref(slot), code, in_ch, view_ch, res, int(max_rows))
    field = torch.empty(res, res, res, device=device, dtype=torch.float32) if 2 <= res <= 1024 else None
    ws = torch.empty(max(nbytes, 256), device=device, dtype=torch.uint8)
    row = torch.empty(L.GRID_STATS, device=device, dtype=torch.float64) if stats else None
    with torch.cuda.device(device):
        L.check(lib.plnerf_density_grid(ctypes.byref(slot), code, in_ch, view_ch, res, L.dptr(tables[0], "xs"), L.dptr(tables[1], "ys"),
                                        L.dptr(tables[2], "zs"), int(max_rows), 1, L.dptr(field, "field"),
                                        L.dptr(row, "stats", torch.float64), ctypes.c_void_p(ws.data_ptr()), nbytes, L.stream()),
                "plnerf_density_grid")
    if status is not None and model.precision in L.GUARDED_PRECISIONS:
        bits = int(status.item())
        if bits:
            status.zero_()
            raise FloatingPointError(f"plnerf_amd: the network left the IEEE-half range on the lattice (status {bits}, "
                                     f"precision={model.precision!r}): the field was clamped.  Use precision='bf16x3' or 'fp32'.")
    del keep
    return field, row


def _block_loop(bound_min, bound_max, resolution, query_func, model):
    """nerf_extract_mesh.py:531-562, statement by statement (without the progress bar).  The mesh script's own run_network
    takes one direction per ROW; run_plnerf.py's -- and this package's -- takes [rays, samples, 3] positions and one direction
    per ray, so a block is handed over as n rays of one sample, which both accept."""
    N = BLOCK
    X, Y, Z = [t.split(N) for t in _linspaces(bound_min, bound_max, resolution)]
    params = list(model.parameters()) if isinstance(model, torch.nn.Module) else []
    u = np.zeros([resolution, resolution, resolution], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    if params:
                        pts = pts.to(params[0].device)
                    viewdirs = torch.zeros_like(pts, device=pts.device)
                    val = query_func(pts[:, None, :], viewdirs, model).reshape(len(xs), len(ys), len(zs), -1)
                    taus = torch.relu(val[..., 3])
                    u[xi * N: xi * N + len(xs), yi * N: yi * N + len(ys), zi * N: zi * N + len(zs)] = taus.detach().cpu().numpy()
    return u


def extract_fields(bound_min, bound_max, resolution, query_func, model, device=False, max_rows=MAX_ROWS_PER_LAUNCH):
    """The reference's extract_fields: relu(raw[..., 3]) of `model` on the resolution^3 lattice between the bounds, as a numpy
    volume [res, res, res] fp32.  One plnerf_density_grid call where the entry serves `model`, else the 64^3 block loop
    through `query_func`.  device=True: the device tensor instead, nothing copied to the host (one-call route only); its
    `grid_stats` attribute is the entry's stats row (min, max, sum, sum of squares: fp64, on the device), which
    extract_iso_level reads."""
    route = _served_route(query_func, model)
    if route is None:
        if device:
            raise ValueError("extract_fields(device=True) needs a network plnerf_density_grid serves (a plnerf_amd.NeRF on the GPU "
                             "that anyview._route admits, queried through create_nerf's network_query_fn)")
        return _block_loop(bound_min, bound_max, resolution, query_func, model)
    xs, ys, zs = _linspaces(bound_min, bound_max, resolution)
    field, stats = density_grid(model, route, xs, ys, zs, max_rows=max_rows, stats=True)
    if device:
        field.grid_stats = stats
        return field
    return field.cpu().numpy()


def extract_iso_level(density, threshold=25, stats=None):
    """The reference's adaptive iso level, min(max(threshold, min + std), max - std).  On a numpy volume: numpy's min / max /
    std, as there.  On a device field: from the stats row of plnerf_density_grid (`stats`, or the field's `grid_stats`) in
    fp64 -- std = sqrt(sumsq / n - (sum / n)^2) -- so the last digits differ from numpy's fp32 `std` of the same volume."""
    if isinstance(density, torch.Tensor):
        stats = stats if stats is not None else getattr(density, "grid_stats", None)
        if stats is None:
            raise ValueError("extract_iso_level on a device field needs the stats row of plnerf_density_grid")
        lo, hi, total, sq = (float(v) for v in stats.detach().cpu().tolist())
        n = density.numel()
        mean = total / n
        min_a, max_a, std_a = lo, hi, float(np.sqrt(max(sq / n - mean * mean, 0.0)))
    else:
        min_a, max_a, std_a = density.min(), density.max(), density.std()
    return min(max(threshold, min_a + std_a), max_a - std_a)


# ---- marching cubes -----------------------------------------------------------------------------------------------------------
def marching_cubes(u, isovalue, device=False):
    """mcubes.marching_cubes' signature and return shapes: (vertices [n_v, 3] fp64 in index coordinates, triangles [n_t, 3]
    int32) of the volume `u` -- a numpy array (uploaded) or a device tensor [nx, ny, nz] -- at `isovalue`, by plnerf_mc_count
    and plnerf_mc_emit.  numpy arrays come back unless device=True.  The counts are read back between the two calls: the one
    synchronisation."""
    if not isinstance(u, torch.Tensor):
        if not torch.cuda.is_available():
            raise RuntimeError("plnerf_amd: marching_cubes runs on the GPU (there is no CPU fallback)")
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda()
    if u.dim() != 3:
        raise ValueError(f"marching_cubes takes a volume [nx, ny, nz], got {tuple(u.shape)}")
    u = u.detach().to(torch.float32).contiguous()
    nx, ny, nz = (int(s) for s in u.shape)
    lib = L.lib()
    nbytes = lib.plnerf_mc_workspace_bytes(nx, ny, nz)
    if nbytes == 0:
        raise ValueError(f"marching_cubes: a lattice of {nx} x {ny} x {nz} is not served (every size >= 2, at most 2^30 points)")
    iso = float(isovalue)
    with torch.cuda.device(u.device):
        ws = torch.empty(nbytes, device=u.device, dtype=torch.uint8)
        counts = torch.empty(2, device=u.device, dtype=torch.int32)
        L.check(lib.plnerf_mc_count(L.dptr(u, "u"), nx, ny, nz, iso, ctypes.c_void_p(ws.data_ptr()), nbytes,
                                    L.dptr(counts, "counts", torch.int32), L.stream()), "plnerf_mc_count")
        n_v, n_t = (int(c) & 0xFFFFFFFF for c in counts.cpu().tolist())
        if max(n_v, n_t) > 2 ** 31 - 1:
            raise OverflowError(f"marching_cubes: {n_v} vertices / {n_t} triangles do not fit int32 indices")
        vertices = torch.empty(n_v, 3, device=u.device, dtype=torch.float64)
        triangles = torch.empty(n_t, 3, device=u.device, dtype=torch.int32)
        L.check(lib.plnerf_mc_emit(L.dptr(u, "u"), nx, ny, nz, iso, ctypes.c_void_p(ws.data_ptr()), nbytes,
                                   ctypes.c_void_p(vertices.data_ptr()) if n_v else None, n_v,
                                   ctypes.c_void_p(triangles.data_ptr()) if n_t else None, n_t, L.stream()), "plnerf_mc_emit")
    if device:
        return vertices, triangles
    return vertices.cpu().numpy(), triangles.cpu().numpy()


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, model, adaptive=False):
    """The reference's extract_geometry (:576-593): the field, the surface at `threshold` (adaptive: at extract_iso_level's
    value), and the vertices rescaled into the bounding box on the host in numpy, by the reference's expression.  Where
    plnerf_density_grid serves `model` the field never leaves the device."""
    if _served_route(query_func, model) is not None:
        u = extract_fields(bound_min, bound_max, resolution, query_func, model, device=True)
    else:
        u = extract_fields(bound_min, bound_max, resolution, query_func, model)
    if not adaptive:
        vertices, triangles = marching_cubes(u, threshold)
    else:
        vertices, triangles = marching_cubes(u, extract_iso_level(u, threshold))
    try:
        b_max_np = bound_max.detach().cpu().numpy()
        b_min_np = bound_min.detach().cpu().numpy()
    except AttributeError:
        b_max_np = bound_max
        b_min_np = bound_min
    vertices = vertices / (resolution - 1.0) * (b_max_np - b_min_np)[None, :] + b_min_np[None, :]
    return vertices, triangles


# ---- floaters, files --------------------------------------------------------------------------------------------------------
def keep_components(triangles, min_len=10000):
    """Bool mask over the faces: those in a component of edge-adjacent faces with at least `min_len` faces -- what
    nerf_extract_mesh.py:1094-1100 keeps through trimesh.graph.connected_components(mesh.face_adjacency, min_len).  Two faces
    are adjacent when they share an edge that exactly two faces use (face_adjacency's rule, from its written description);
    a face adjacent to none is in no component.  numpy only."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    F = len(t)
    mask = np.zeros(F, dtype=bool)
    if F == 0:
        return mask
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    face = np.tile(np.arange(F), 3)
    key = edges[:, 0] * (int(t.max()) + 1) + edges[:, 1]
    order = np.argsort(key, kind="stable")
    key, face = key[order], face[order]
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    size = np.diff(np.concatenate([start, [len(key)]]))
    first = start[size == 2]
    a, b = face[first], face[first + 1]
    ok = a != b
    a, b = a[ok], b[ok]
    adjacent = np.zeros(F, dtype=bool)
    adjacent[a] = adjacent[b] = True
    label = np.arange(F)
    while True:      # the smallest face index of the component, by propagation along the pairs and pointer jumping
        new = label.copy()
        np.minimum.at(new, a, label[b])
        np.minimum.at(new, b, label[a])
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    counts = np.bincount(label[adjacent], minlength=F)
    mask[adjacent] = counts[label[adjacent]] >= min_len
    return mask


_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
               "element face {}\nproperty list uchar int vertex_indices\nend_header\n")
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, vertices, triangles):
    """A triangle mesh as a binary little-endian PLY file: float32 positions, int32 face indices."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype="<f4").reshape(-1, 3))
    t = np.asarray(triangles).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_ply: a face names a vertex that is not there")
    faces = np.empty(len(t), dtype=_PLY_FACE)
    faces["n"] = 3
    faces["v"] = t
    with open(path, "wb") as f:
        f.write(_PLY_HEADER.format(len(v), len(t)).encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """(vertices [n, 3] float32, triangles [m, 3] int32) of a file write_ply wrote."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or lines[2:] != _PLY_HEADER.format(
            lines[2].split()[-1], lines[6].split()[-1]).split("\n")[2:]:
        raise ValueError("read_ply reads what write_ply writes: binary little-endian, float x y z, uchar / int faces")
    n, m = int(lines[2].split()[-1]), int(lines[6].split()[-1])
    if len(data) != end + 12 * n + _PLY_FACE.itemsize * m:
        raise ValueError("read_ply: the file's length does not match its header")
    v = np.frombuffer(data, dtype="<f4", count=3 * n, offset=end).reshape(n, 3).copy()
    faces = np.frombuffer(data, dtype=_PLY_FACE, count=m, offset=end + 12 * n)
    if m and not (faces["n"] == 3).all():
        raise ValueError("read_ply: a face that is not a triangle")
    return v, faces["v"].astype(np.int32)
