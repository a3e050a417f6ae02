"""The cases of tests/test_gpu_mesh.py on tests/containment.py's descriptions (Buf / Call / Struct; run_case carries a case out
on a sentinel arena with the scratch at 0x00, at 0xFF -- NaN bit patterns -- and on ordinary allocations, and holds the three
runs to each other), built without a GPU: tests/test_mesh_abi.py builds every one of them on the CPU.

    grid_case   plnerf_mlp_pack_weights + plnerf_mlp_fwd on the lattice's positions (the network's existing forward), then
                plnerf_density_grid on the same packed weights under several max_rows, each into a field and a stats row of its own
    mc_case     plnerf_mc_count, then plnerf_mc_emit into arrays of the sizes tests/mesh_model.py says (or one row short)
"""
import ctypes

import numpy as np
import torch

import containment as C
import mesh_model

RESOLUTION = 21                      # 9,261 rows: no multiple of the 128- or 256-row forward tiles
MAX_ROWS = (100, 1000, 10000)        # blocks cut inside a tile, inside the lattice, and one block (>= 9,261)
BOUNDS = ((-1.5, 1.25), (-1.0, 1.5), (-1.25, 1.0))


def lattice(resolution, bounds=BOUNDS):
    """(xs, ys, zs) as the caller's torch.linspace, and the [res^3, 3] positions in the field's index order."""
    tables = [torch.linspace(lo, hi, resolution) for lo, hi in bounds]
    xx, yy, zz = torch.meshgrid(*tables, indexing="ij")
    return tables, torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1).contiguous()


def _density_without_bias(flat, offs, counts, pts):
    """alpha_linear.weight . h of the 8 x 256 trunk (skip behind layer 4, 10 bands) at `pts`, in plain torch."""
    shapes = C.param_shapes(63, 27)
    tensor = lambda k: flat[offs[k] // 4: offs[k] // 4 + counts[k]].reshape(shapes[k])
    enc = torch.cat([pts] + [fn(pts * 2.0 ** f) for f in range(10) for fn in (torch.sin, torch.cos)], -1)
    h = enc
    for layer in range(8):
        h = torch.relu(torch.nn.functional.linear(h, tensor(2 * layer), tensor(2 * layer + 1)))
        if layer == 4:
            h = torch.cat([enc, h], -1)
    return torch.nn.functional.linear(h, tensor(20))[:, 0]


def _slot(L, flat, offs, packed):
    def build(addr):
        net = L.AnyViewNet()
        net.route = L.ANYVIEW_FUSED
        base = addr(C.IN(flat))
        for k, o in enumerate(offs):
            net.fused.params[k] = base + o
        net.fused.packed = addr(C.OUT(packed))
        return net
    return C.Struct([C.IN(flat), C.OUT(packed)], build)


def grid_case(L, precision, resolution=RESOLUTION, max_rows=MAX_ROWS, tag=""):
    """Returns (calls, names): names["ref"] the raw [n, 4] of plnerf_mlp_fwd, names["fields"] / ["stats"] one per max_rows."""
    P = C.PRECISIONS[precision]
    t = f"{tag}{precision}_r{resolution}_"
    flat, offs, counts = C.network(t, 63, 27)
    packed = C._packed(L, t, P)
    tables, pts = lattice(resolution)
    # alpha_linear.bias: minus the median of the density's other terms on the lattice (fp32 torch on the CPU), so that about
    # half the lattice lies on either side of the relu
    flat.data[offs[21] // 4] = -float(_density_without_bias(flat.data, offs, counts, pts).median())
    n = pts.shape[0]
    xs, ys, zs = (C.given(f"{t}{a}s", "f32", v) for a, v in zip("xyz", tables))
    pts_b = C.given(f"{t}pts", "f32", pts)
    dirs = C.given(f"{t}dirs", "f32", torch.zeros(n, 3))
    ref = C.out(f"{t}ref_raw", "f32", n, 4, align=16)
    slot = _slot(L, flat, offs, packed)
    calls = [
        C.Call("plnerf_mlp_pack_weights", C.PtrTable([C.IN(flat, o) for o in offs]), P, 63, 27, C.OUT(packed)),
        C.Call("plnerf_mlp_fwd", C.IN(packed), P, C.IN(pts_b), C.IN(dirs), None, 63, 27, n, 1, 1.0, 0.0, C.OUT(ref), None, C.KERNEL_AUTO),
    ]
    names = {"ref": ref.name, "fields": [], "stats": [], "n": n}
    for k, rows in enumerate(max_rows):
        nbytes = int(L.lib().plnerf_density_grid_workspace_bytes(ctypes.byref(slot.build(lambda r: 1 << 20)), P, 63, 27, resolution, rows))
        assert nbytes > 0, (precision, resolution, rows)
        ws = C.out(f"{t}ws{rows}", "u8", nbytes, align=256, opaque=True)
        field = C.out(f"{t}field{rows}", "f32", n)
        stats = C.out(f"{t}stats{rows}", "f64", L.GRID_STATS)
        # (the first call packs the weights again: pack_weights = 1; the others read the packed buffer as it is)
        calls.append(C.Call("plnerf_density_grid", slot, P, 63, 27, resolution, C.IN(xs), C.IN(ys), C.IN(zs), rows, 1 if k == 0 else 0,
                            C.OUT(field), C.OUT(stats), C.SCRATCH(ws), nbytes))
        names["fields"].append(field.name)
        names["stats"].append(stats.name)
    return calls, names


# ---- marching cubes -----------------------------------------------------------------------------------------------------------
def mc_fields():
    """{name: (field, iso)}: the CPU test's fields, a 2 x 3 x 5 lattice, a single cell, nothing inside, everything inside,
    values exactly equal to iso at lattice points, and the two sizes at which the launches take another path."""
    rng = np.random.default_rng(11)
    out = {f"noise{s}": (mesh_model.noise_field(s), 0.0) for s in mesh_model.NOISE_SEEDS}
    out["sphere"] = (mesh_model.sphere_field(), 0.0)
    out["2x3x5"] = ((rng.random((2, 3, 5)) * 2 - 1).astype(np.float32), 0.125)
    out["cell"] = (np.array([[[0.5, -1.0], [-0.25, 2.0]], [[-3.0, 0.75], [1.5, -0.5]]], dtype=np.float32), 0.1)
    out["outside"] = (np.full((4, 5, 3), -1.0, dtype=np.float32), 0.0)
    out["inside"] = (np.full((3, 4, 5), 2.0, dtype=np.float32), 0.0)
    quantised = np.round(mesh_model.noise_field(5, n=8) * 2) / 2      # multiples of 0.5 in [-1, 1]: a third of the points AT iso
    out["at_iso"] = (quantised.astype(np.float32), 0.5)
    # 1,100 points in one row: two workgroups of 1,024, and an x stride of one row
    out["two_blocks"] = ((rng.random((2, 2, 275)) * 2 - 1).astype(np.float32), 0.0)
    # 1,064,960 points: 1,040 blocks, so a second group of 1,024 blocks -- the size at which the second scan level has work
    x, y, z = np.meshgrid(np.arange(130), np.arange(128), np.arange(64), indexing="ij")
    out["two_groups"] = ((np.sin(x / 5.0) + np.sin(y / 7.0) + np.sin(z / 3.0)).astype(np.float32), 0.25)
    return out


def mc_case(L, name, field, iso, short=False):
    """Returns (calls, names, (expected vertices, expected triangles)).  short: capacities one row below the counts -- the last
    row of either array must stay untouched."""
    nx, ny, nz = field.shape
    want_v, want_t = mesh_model.marching_cubes(field, iso)
    n_v, n_t = len(want_v), len(want_t)
    t = f"mc_{name}_{'short_' if short else ''}"
    nbytes = int(L.lib().plnerf_mc_workspace_bytes(nx, ny, nz))
    assert nbytes > 0
    f = C.given(f"{t}field", "f32", torch.from_numpy(field))
    ws = C.out(f"{t}ws", "u8", nbytes, align=256, opaque=True)
    counts = C.out(f"{t}counts", "u32", 2)
    calls = [C.Call("plnerf_mc_count", C.IN(f), nx, ny, nz, float(iso), C.SCRATCH(ws), nbytes, C.OUT(counts))]
    names = {"counts": counts.name, "vertices": None, "triangles": None}
    if n_v == 0:
        assert n_t == 0 and not short
        calls.append(C.Call("plnerf_mc_emit", C.IN(f), nx, ny, nz, float(iso), C.IN(ws), nbytes, None, 0, None, 0))
        return calls, names, (want_v, want_t)
    assert n_t > 0 and (not short or (n_v > 1 and n_t > 1))
    last_v = torch.zeros(n_v, 6, dtype=torch.bool)      # (words: an fp64 is two)
    last_t = torch.zeros(n_t, 3, dtype=torch.bool)
    last_v[-1], last_t[-1] = True, True
    vertices = C.out(f"{t}vertices", "f64", n_v, 3, untouched=last_v if short else None, finite=not short)      # (the fill is a NaN)
    triangles = C.out(f"{t}triangles", "i32", n_t, 3, untouched=last_t if short else None)
    calls.append(C.Call("plnerf_mc_emit", C.IN(f), nx, ny, nz, float(iso), C.IN(ws), nbytes, C.OUT(vertices), n_v - int(short),
                        C.OUT(triangles), n_t - int(short)))
    names.update(vertices=vertices.name, triangles=triangles.name)
    return calls, names, (want_v, want_t)
