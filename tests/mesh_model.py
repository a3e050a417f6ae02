"""plnerf_mc_count / plnerf_mc_emit (include/experimental/plnerf_hip_mesh.h) restated in numpy ON THE COMMITTED TABLE
(pl-nerf_amd/csrc/mc_table.h, parsed here), and the invariants that vouch for that table.

The model shares the table with the kernel, so agreement between the two says nothing about the table.  What does: the
check_* functions at the end of this file (tests/test_mesh_table_host.py calls them: pytest collects test_*.py only), which
hold the meshes the model builds to combinatorial invariants -- every mesh edge in exactly two triangles, traversed in opposite
directions; a sphere is one closed surface of Euler characteristic 2 with positive signed volume (normals towards decreasing
field) -- over fields whose cells together take all 256 states.

Conventions restated from the header: a corner is inside when f >= iso (NaN: outside); a lattice edge crosses when exactly one
end is inside; the vertex on the edge from point p along axis a lies at p_a + (iso - f1) / (f2 - f1), evaluated in fp64 from the
fp32 values (f1 at p); vertices are ordered by owning lattice point (linear index (x ny + y) nz + z), then axis; triangles by
cell (the linear index of its lattice point), then table order."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_HEADER = os.path.join(ROOT, "pl-nerf_amd", "csrc", "mc_table.h")


def load_table(path=TABLE_HEADER):
    """(ntri [256], tri [256, row]) as the header holds them."""
    code = re.sub(r"//[^\n]*", "", open(path).read())
    ntri = re.search(r"plnerf_mc_ntri\[256\]\s*=\s*\{(.*?)\};", code, flags=re.S).group(1)
    tri = re.search(r"plnerf_mc_tri\[256\]\[PLNERF_MC_ROW\]\s*=\s*\{(.*)\};", code, flags=re.S).group(1)
    row = int(re.search(r"#define PLNERF_MC_ROW (\d+)", code).group(1))
    ntri = np.array([int(v) for v in ntri.replace(",", " ").split()], dtype=np.int64)
    tri = np.array([int(v) for v in re.sub(r"[{},]", " ", tri).split()], dtype=np.int64).reshape(256, row)
    assert ntri.shape == (256,)
    return ntri, tri


def edge_owner(e):
    """(offsets of edge e's owning corner, axis): tools/gen_mc_table.py's numbering, restated."""
    a, k = divmod(int(e), 4)
    b, c = [x for x in range(3) if x != a]
    off = [0, 0, 0]
    off[b], off[c] = k & 1, k >> 1
    return tuple(off), a


def cell_states(field, iso):
    """[nx - 1, ny - 1, nz - 1] states: bit i = corner (i & 1, (i >> 1) & 1, (i >> 2) & 1) inside."""
    inside = field.astype(np.float64) >= float(iso)
    nx, ny, nz = field.shape
    state = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for i in range(8):
        dx, dy, dz = i & 1, (i >> 1) & 1, (i >> 2) & 1
        state |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << i
    return state


def marching_cubes(field, iso, table=None):
    """(vertices [n_v, 3] fp64 in index coordinates, triangles [n_t, 3] int32) of an fp32 field [nx, ny, nz]."""
    ntri, tri = table if table is not None else load_table()
    field = np.ascontiguousarray(field, dtype=np.float32)
    nx, ny, nz = field.shape
    iso = float(iso)
    f64 = field.astype(np.float64)
    inside = f64 >= iso
    # crossing flags per lattice point and axis, in the order the vertices are numbered
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    index = (np.cumsum(cross.reshape(-1)) - 1).reshape(nx, ny, nz, 3)      # vertex index where cross is set
    px, py, pz, pa = np.nonzero(cross)                                     # (row-major: point, then axis)
    p = np.stack([px, py, pz], 1)
    q = p.copy()
    q[np.arange(len(pa)), pa] += 1
    f1, f2 = f64[px, py, pz], f64[q[:, 0], q[:, 1], q[:, 2]]
    with np.errstate(all="ignore"):
        t = (iso - f1) / (f2 - f1)
    vertices = p.astype(np.float64)
    vertices[np.arange(len(pa)), pa] = p[np.arange(len(pa)), pa].astype(np.float64) + t
    # triangles, cell by cell
    state = cell_states(field, iso)
    count = ntri[state].reshape(-1)
    start = np.cumsum(count) - count
    triangles = np.zeros((int(count.sum()), 3), dtype=np.int32)
    cx, cy, cz = [v.reshape(-1) for v in np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")]
    flat_state = state.reshape(-1)
    for k in range(int(count.max()) if count.size else 0):
        sel = np.nonzero(count > k)[0]
        for j in range(3):
            edges = tri[flat_state[sel], 3 * k + j]
            offs = np.array([edge_owner(e)[0] for e in range(12)])[edges]
            axes = np.array([edge_owner(e)[1] for e in range(12)])[edges]
            triangles[start[sel] + k, j] = index[cx[sel] + offs[:, 0], cy[sel] + offs[:, 1], cz[sel] + offs[:, 2], axes]
    return vertices, triangles


# ---- the fields of the tests (CPU and GPU) ------------------------------------------------------------------------------
NOISE_SEEDS = (1, 2, 3, 4, 5, 6, 7)      # chosen on the CPU: together all 256 states (checked below)


def noise_field(seed, n=9):
    """White noise in [-1, 1) on n^3 with a border below iso = 0: the surface is closed."""
    rng = np.random.default_rng(seed)
    f = (rng.random((n, n, n)) * 2 - 1).astype(np.float32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    return f


def sphere_field(n=17, radius=5.3, centre=(7.9, 8.2, 8.4)):
    """radius - |p - centre|: positive inside a sphere that stays clear of the border; iso = 0."""
    x, y, z = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (radius - d).astype(np.float32)


def two_spheres_field():
    """Two disjoint spheres in one 24 x 15 x 15 lattice: a 15^3 one and a 7^3 one side by side (tests of keep_components)."""
    f = np.full((24, 15, 15), -1.0, dtype=np.float32)
    f[:15] = sphere_field(15, 5.2, (7.1, 6.9, 7.2))
    small = sphere_field(7, 2.1, (3.1, 2.9, 3.2))
    f[16:23, 4:11, 4:11] = small
    return f


# ---- invariants ----------------------------------------------------------------------------------------------------------
def directed_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def assert_closed_and_oriented(triangles):
    """Every mesh edge belongs to exactly two triangles, which traverse it in opposite directions."""
    e = directed_edges(triangles)
    assert (e[:, 0] != e[:, 1]).all()
    key = e[:, 0] * (e.max() + 1) + e[:, 1]
    back = e[:, 1] * (e.max() + 1) + e[:, 0]
    assert len(np.unique(key)) == len(key), "a directed edge is used twice"
    assert np.array_equal(np.sort(key), np.sort(back)), "an edge lacks its opposite"


def components(triangles, n_vertices):
    """Number of vertex-connected components among the vertices the triangles use."""
    parent = np.arange(n_vertices)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in directed_edges(triangles):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return len({find(v) for v in np.unique(triangles)})


def signed_volume(vertices, triangles):
    v0, v1, v2 = (vertices[triangles[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6.0)


def check_noise_meshes_are_closed_and_oriented():
    for seed in NOISE_SEEDS:
        v, t = marching_cubes(noise_field(seed), 0.0)
        assert len(t) > 100 and t.max() == len(v) - 1 and len(np.unique(t)) == len(v)
        assert_closed_and_oriented(t)


def check_sphere_is_one_closed_surface_with_outward_normals():
    v, t = marching_cubes(sphere_field(), 0.0)
    assert_closed_and_oriented(t)
    E = len(directed_edges(t)) // 2
    assert components(t, len(v)) == 1 and len(v) - E + len(t) == 2
    vol = signed_volume(v, t)
    assert 0.9 * 4 / 3 * np.pi * 5.3 ** 3 < vol < 4 / 3 * np.pi * 5.3 ** 3, vol      # (positive: normals leave the dense region)


def check_the_fields_reach_every_state():
    seen = set()
    for f in [noise_field(s) for s in NOISE_SEEDS] + [sphere_field()]:
        seen |= set(np.unique(cell_states(f, 0.0)).tolist())
    assert seen == set(range(256)), sorted(set(range(256)) - seen)
