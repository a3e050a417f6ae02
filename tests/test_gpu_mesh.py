"""Mesh extraction (include/experimental/plnerf_hip_mesh.h, plnerf_amd.mesh) on a real MI355X.

Every check is exact or a bound derived here.  plnerf_density_grid: bit for bit relu(raw[:, 3]) of the network's existing forward
on the same positions (plnerf_mlp_fwd through the raw ABI for the compiled trunk, run_network -> generic.forward for a CHAIN16
and a LAYERS32 slot), equal across max_rows, on workspaces filled with 0x00 and with 0xFF bytes (NaN bit patterns) inside
guard-banded arenas; its stats row against the field.  plnerf_mc_count / plnerf_mc_emit: counts, vertex bytes and triangle ints
equal to tests/mesh_model.py's on the CPU test's fields and the edge cases of tests/mesh_cases.py, three runs identical, nothing
written past capacities one short of the counts.  extract_geometry end to end against the Python block loop + mesh_model."""
import contextlib
import math

import numpy as np
import pytest
import torch

import containment as C
import generic_cases
import mesh_cases
import mesh_model
from gpu_support import P, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from plnerf_amd import _lib
    return _lib


def _f32(run, name):
    return run[name].view(torch.float32)


def _relu_bits_equal(field, raw):
    """field == relu(raw[:, 3]) bit for bit (a zero of either sign is a zero: torch.relu keeps -0.0's sign on some paths)."""
    want = torch.relu(raw.reshape(-1, 4)[:, 3])
    nonzero = want != 0
    return (torch.equal(field, want) and torch.equal(field[nonzero].view(torch.int32), want[nonzero].view(torch.int32))
            and bool((field >= 0).all()))


# ----------------------------------------------------------------------------- the density lattice
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3", "fp32"])
def test_density_grid_is_the_forward_on_the_lattice(L, precision):
    calls, names = mesh_cases.grid_case(L, precision)
    run = C.run_case(L, calls, dev())
    raw = _f32(run, names["ref"])
    fields = [_f32(run, f) for f in names["fields"]]
    assert 0.05 < float((fields[0] > 0).float().mean()) < 0.95      # the relu matters on this lattice
    assert _relu_bits_equal(fields[0], raw)
    for f in fields[1:]:      # the field does not depend on max_rows
        assert torch.equal(f.view(torch.int32), fields[0].view(torch.int32))
    # ---- the stats row against fp64 numpy of the field
    # min and max: exact.  sum and sum of squares: the device adds n = 9,261 non-negative fp64 terms in SOME fixed order; any
    # order of recursive or pairwise summation of n terms obeys |computed - exact| <= gamma(n - 1) sum |x_i| with
    # gamma(k) = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability, eq. 4.4).  The terms themselves are exact: an
    # fp32 value is an fp64 value, and the square of a 24-bit significand has 48 bits.  The reference is math.fsum, the
    # correctly rounded exact sum: one more u.  So the bound is (gamma(n - 1) + u) * sum.
    x = fields[0].double().numpy()
    n, u = x.size, 2.0 ** -53
    bound = ((n - 1) * u / (1 - (n - 1) * u) + u)
    exact_sum, exact_sq = math.fsum(x.tolist()), math.fsum((x * x).tolist())
    for name in names["stats"]:
        s = run[name].view(torch.float64).numpy()
        print(precision, name, s, "sum err", abs(s[L.GRID_SUM] - exact_sum) / exact_sum, "sq err", abs(s[L.GRID_SUMSQ] - exact_sq) / exact_sq,
              "bound", bound)
        assert s[L.GRID_MIN] == x.min() and s[L.GRID_MAX] == x.max()
        assert abs(s[L.GRID_SUM] - exact_sum) <= bound * exact_sum
        assert abs(s[L.GRID_SUMSQ] - exact_sq) <= bound * exact_sq


def test_density_grid_at_resolution_two(L):
    calls, names = mesh_cases.grid_case(L, "f16x3", resolution=2, max_rows=(3, 8))
    run = C.run_case(L, calls, dev())
    assert names["n"] == 8
    for f in names["fields"]:
        assert _relu_bits_equal(_f32(run, f), _f32(run, names["ref"]))


@contextlib.contextmanager
def _honouring(on):
    from plnerf_amd import generic
    found, generic.HONOUR_PRECISION = generic.HONOUR_PRECISION, on
    try:
        yield
    finally:
        generic.HONOUR_PRECISION = found


@pytest.mark.parametrize("route", ["chain16", "layers32"])
def test_density_grid_on_a_slot_outside_the_trunk(P, L, route):
    """Resolution 9 (729 rows, blocks of 100) on generic_cases.SHAPES[1] (netdepth 12, netwidth 96, three skips, 5 | 2 bands)
    against run_network, which reaches generic.forward, on the same positions with a zero direction."""
    from plnerf_amd import mesh
    chain = route == "chain16"
    with _honouring(chain):
        net, emb, embd = generic_cases.build(P, generic_cases.SHAPES[1], "f16x3" if chain else "fp32")
        with torch.no_grad():
            net.alpha_linear.bias.zero_()
        got_route = mesh.anyview._route(net, (emb, embd))[0]
        assert got_route == (L.ANYVIEW_CHAIN16 if chain else L.ANYVIEW_LAYERS32)
        tables, pts = mesh_cases.lattice(9)
        pts = pts.to(dev())
        with torch.no_grad():
            raw = P.run_network(pts[:, None, :], torch.zeros_like(pts), net, emb, embd)
        field, stats = mesh.density_grid(net, got_route, *tables, max_rows=100)
        whole, _ = mesh.density_grid(net, got_route, *tables, max_rows=1 << 20, stats=False)
        torch.cuda.synchronize()
    assert 0.02 < float((field > 0).float().mean()) < 0.98
    assert _relu_bits_equal(field.reshape(-1), raw.reshape(-1, 4))
    assert torch.equal(whole.view(torch.int32), field.view(torch.int32))
    s = stats.cpu().numpy()
    assert s[L.GRID_MIN] == float(field.min()) and s[L.GRID_MAX] == float(field.max())


# ----------------------------------------------------------------------------- marching cubes
def _check_mesh(L, name, field, iso, short=False):
    calls, names, (want_v, want_t) = mesh_cases.mc_case(L, name, field, iso, short=short)
    run = C.run_case(L, calls, dev())      # (three runs, held equal byte for byte: "two runs identical")
    counts = run[names["counts"]].view(torch.int32).tolist()
    assert counts == [len(want_v), len(want_t)], (name, counts)
    if names["vertices"] is None:
        return
    keep_v, keep_t = len(want_v) - int(short), len(want_t) - int(short)
    got_v = run[names["vertices"]].view(torch.int64).reshape(-1, 3).numpy()
    got_t = run[names["triangles"]].view(torch.int32).reshape(-1, 3).numpy()
    assert np.array_equal(got_v[:keep_v], want_v.view(np.int64)[:keep_v]), name      # the vertex BYTES
    assert np.array_equal(got_t[:keep_t], want_t[:keep_t]), name


@pytest.mark.parametrize("name", sorted(mesh_cases.mc_fields()))
def test_marching_cubes_is_the_model(L, name):
    field, iso = mesh_cases.mc_fields()[name]
    _check_mesh(L, name, field, iso)


def test_emit_writes_nothing_past_short_capacities(L):
    field, iso = mesh_cases.mc_fields()["sphere"]
    _check_mesh(L, "sphere", field, iso, short=True)      # (run_case: the last rows still hold the fill, the guards are intact)


def test_marching_cubes_takes_numpy_and_device_volumes(P):
    field, iso = mesh_cases.mc_fields()["noise2"]
    want_v, want_t = mesh_model.marching_cubes(field, iso)
    for u in (field, torch.from_numpy(field).to(dev())):
        v, t = P.marching_cubes(u, iso)
        assert v.dtype == np.float64 and t.dtype == np.int32 and v.shape == want_v.shape and t.shape == want_t.shape
        assert np.array_equal(v.view(np.int64), want_v.view(np.int64)) and np.array_equal(t, want_t)
    v, t = P.marching_cubes(np.full((3, 3, 3), -1.0, dtype=np.float32), 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)


# ----------------------------------------------------------------------------- end to end
def test_extract_geometry_end_to_end(P):
    """A default-initialised fused network at resolution 17, threshold = the median of the positive field: the device route
    (plnerf_density_grid -> plnerf_mc_count / _emit -> the host rescale) against the Python block loop + mesh_model."""
    from plnerf_amd import mesh
    torch.manual_seed(3)
    net = P.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True, precision="f16x3").to(dev())
    emb, embd = P.get_embedder(10, 0)[0], P.get_embedder(4, 0)[0]

    def query(inputs, viewdirs, fn):
        return P.run_network(inputs, viewdirs, fn, emb, embd)
    query.embedders = (emb, embd)
    bound_min, bound_max, res = np.array([-1.2, -1.0, -0.9]), np.array([1.1, 1.3, 1.0]), 17
    assert mesh._served_route(query, net) == 0      # PLNERF_ANYVIEW_FUSED
    u = mesh._block_loop(bound_min, bound_max, res, query, net)
    positive = u[u > 0]
    assert positive.size > 100, positive.size
    threshold = float(np.median(positive))
    want_v, want_t = mesh_model.marching_cubes(u, threshold)
    assert len(want_t) > 0      # a surface exists -- checked on the CPU side before anything is asserted about it
    want_v = want_v / (res - 1.0) * (bound_max - bound_min)[None, :] + bound_min[None, :]
    # the one-call field is the block loop's, bit for bit
    field = P.extract_fields(bound_min, bound_max, res, query, net)
    assert field.dtype == np.float32 and np.array_equal(field.view(np.int32), u.view(np.int32))
    v, t = P.extract_geometry(bound_min, bound_max, res, threshold, query, net)
    assert np.array_equal(v.view(np.int64), want_v.view(np.int64)) and np.array_equal(t, want_t)
    # the device field's iso level: from the stats row in fp64, numpy's from the volume in fp32 -- equal to rounding
    on_device = P.extract_fields(bound_min, bound_max, res, query, net, device=True)
    assert on_device.is_cuda and on_device.shape == (res, res, res)
    for thr in (0.0, threshold, 1e9):
        a, b = P.extract_iso_level(on_device, thr), float(P.extract_iso_level(u, thr))
        assert abs(a - b) <= 1e-5 * max(abs(b), 1e-6), (thr, a, b)
    # a model the entry does not serve goes through the block loop (here: the query function does not name its encoders)
    plain = lambda inputs, viewdirs, fn: query(inputs, viewdirs, fn)
    assert mesh._served_route(plain, net) is None
    assert np.array_equal(P.extract_fields(bound_min, bound_max, res, plain, net).view(np.int32), u.view(np.int32))
