"""The host side of plnerf_amd.mesh, without a GPU: the PLY writer and its reader, keep_components on two disjoint spheres,
extract_geometry's rescale against the reference's expression, extract_iso_level's three branches on a numpy volume, and that
nothing here falls back to a CPU kernel."""
import numpy as np
import pytest
import torch

import mesh_model
from plnerf_amd import mesh


def test_exports():
    import plnerf_amd
    for name in ("extract_fields", "extract_geometry", "extract_iso_level", "marching_cubes", "keep_components", "write_ply", "read_ply"):
        assert getattr(plnerf_amd, name) is getattr(mesh, name) and name in plnerf_amd.__all__, name


def test_ply_round_trip(tmp_path):
    v, t = mesh_model.marching_cubes(mesh_model.sphere_field(), 0.0)
    path = tmp_path / "sphere.ply"
    mesh.write_ply(path, v, t)
    data = path.read_bytes()
    head = data[:data.index(b"end_header\n") + 11].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    assert head[3:6] == ["property float x", "property float y", "property float z"]
    assert head[6:8] == [f"element face {len(t)}", "property list uchar int vertex_indices"]
    assert len(data) == len("\n".join(head)) + 12 * len(v) + 13 * len(t)      # float32 positions; a count byte + three int32 per face
    v2, t2 = mesh.read_ply(path)
    assert v2.dtype == np.float32 and t2.dtype == np.int32
    assert np.array_equal(v2, v.astype(np.float32)) and np.array_equal(t2, t)
    # the empty mesh, and a face that names a vertex that is not there
    mesh.write_ply(path, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32))
    v0, t0 = mesh.read_ply(path)
    assert v0.shape == (0, 3) and t0.shape == (0, 3)
    with pytest.raises(ValueError, match="not there"):
        mesh.write_ply(path, v[:5], t)
    path.write_bytes(data[:-1])
    with pytest.raises(ValueError, match="length"):
        mesh.read_ply(path)


def test_keep_components_on_two_disjoint_spheres():
    """A sphere in a 15^3 lattice and one in a 7^3 lattice, side by side: min_len between their face counts keeps the large one."""
    v, t = mesh_model.marching_cubes(mesh_model.two_spheres_field(), 0.0)
    large = v[t[:, 0], 0] < 15.5      # (a face's component by where it lies along x)
    n_large, n_small = int(large.sum()), int((~large).sum())
    assert n_large > n_small > 50 and mesh_model.components(t, len(v)) == 2
    assert np.array_equal(mesh.keep_components(t, min_len=(n_large + n_small) // 2), large)
    assert mesh.keep_components(t, min_len=n_small).all() and mesh.keep_components(t, min_len=1).all()
    assert np.array_equal(mesh.keep_components(t, min_len=n_small + 1), large)
    assert np.array_equal(mesh.keep_components(t, min_len=n_large), large)
    assert not mesh.keep_components(t, min_len=n_large + 1).any()
    assert mesh.keep_components(t).dtype == bool and not mesh.keep_components(t).any()      # the reference's 10,000
    # a face adjacent to none is in no component; the order of the faces does not matter
    lone = np.concatenate([t, [[0, 1, len(v) + 5]]])
    assert not mesh.keep_components(lone, min_len=1)[-1] and mesh.keep_components(lone, min_len=1)[:-1].all()
    perm = np.random.default_rng(0).permutation(len(t))
    assert np.array_equal(mesh.keep_components(t[perm], min_len=n_small + 1), large[perm])
    assert mesh.keep_components(np.zeros((0, 3), dtype=np.int32)).shape == (0,)


def test_extract_geometry_rescales_by_the_reference_expression(monkeypatch):
    """(:591) vertices / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :], in numpy on the host: the field and
    the surface are stood in for, the bounds given as numpy arrays and as tensors."""
    rng = np.random.default_rng(4)
    fixed_v = rng.random((37, 3)) * 16.0
    fixed_t = rng.integers(0, 37, (20, 3)).astype(np.int32)
    seen = {}
    monkeypatch.setattr(mesh, "_served_route", lambda query_func, model: None)
    monkeypatch.setattr(mesh, "extract_fields", lambda *a, **k: np.arange(8, dtype=np.float32).reshape(2, 2, 2))

    def surface(u, iso):
        seen["iso"] = iso
        return fixed_v.copy(), fixed_t.copy()
    monkeypatch.setattr(mesh, "marching_cubes", surface)
    b_min, b_max = np.array([-1.25, -0.5, 0.3]), np.array([1.0, 2.5, 0.9])
    want = fixed_v / (17 - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
    for lo, hi in ((b_min, b_max), (torch.from_numpy(b_min), torch.from_numpy(b_max))):
        v, t = mesh.extract_geometry(lo, hi, 17, 25, None, None)
        assert np.array_equal(v.view(np.int64), want.view(np.int64)) and np.array_equal(t, fixed_t) and seen["iso"] == 25
    mesh.extract_geometry(b_min, b_max, 17, 25, None, None, adaptive=True)
    assert seen["iso"] == mesh.extract_iso_level(np.arange(8, dtype=np.float32), 25)


def test_extract_iso_level_on_a_numpy_volume():
    """min(max(threshold, min + std), max - std) with numpy's min / max / std: each of the three values wins once."""
    u = np.array([0.0, 1.0, 50.0, 100.0], dtype=np.float32).reshape(1, 2, 2)
    lo, hi, std = u.min(), u.max(), u.std()
    assert lo + std < 50 < hi - std
    assert mesh.extract_iso_level(u, 50) == 50                      # the threshold itself
    assert mesh.extract_iso_level(u, 25) == lo + std                # below min + std
    assert mesh.extract_iso_level(u, 90) == hi - std                # above max - std
    assert mesh.extract_iso_level(u) == mesh.extract_iso_level(u, 25)
    # on a device field the stats row is needed (here: a CPU tensor stands for it; nothing is computed on it)
    t = torch.from_numpy(u)
    with pytest.raises(ValueError, match="stats row"):
        mesh.extract_iso_level(t, 25)
    x = u.astype(np.float64)
    stats = torch.tensor([x.min(), x.max(), x.sum(), (x * x).sum()], dtype=torch.float64)
    for thr in (25, 50, 90):
        assert abs(mesh.extract_iso_level(t, thr, stats=stats) - float(mesh.extract_iso_level(u, thr))) < 1e-4


def test_there_is_no_cpu_fallback():
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mesh.marching_cubes(mesh_model.sphere_field(), 0.0)
    # without a network the entry serves, extract_fields is the block loop through query_func (any callable, any model)
    calls = []

    def query(pts, viewdirs, model):
        calls.append((tuple(pts.shape), tuple(viewdirs.shape)))
        assert not viewdirs.any()
        return torch.cat([torch.zeros(pts.shape[0], 1, 3), pts.sum(-1, keepdim=True)], -1)
    u = mesh.extract_fields(np.array([-1.0, -1.0, -1.0]), np.array([1.0, 2.0, 3.0]), 5, query, None)
    xs, ys, zs = (np.linspace(-1, hi, 5, dtype=np.float32) for hi in (1.0, 2.0, 3.0))
    want = np.maximum(xs[:, None, None] + ys[None, :, None] + zs[None, None, :], 0)
    assert u.dtype == np.float32 and u.shape == (5, 5, 5) and np.allclose(u, want, atol=1e-6) and calls == [((125, 1, 3), (125, 3))]
    with pytest.raises(ValueError, match="device=True"):
        mesh.extract_fields(np.zeros(3), np.ones(3), 5, query, None, device=True)
