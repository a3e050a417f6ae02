"""generic.CHAIN_INFERENCE and include/experimental/plnerf_hip_generic.h: the layer-by-layer route's no-grad forward as one
plnerf_generic_fwd call on 16-bit activation planes.  The oracle is the route it replaces: generic.HONOUR_PRECISION's
plnerf_gemm_h16 per layer, BIT FOR BIT (tests/test_gpu_generic_precision.py holds that route to fp64).  Also the packed-row
format on its own (plnerf_pack_h16 against torch's conversions), the independence of a row from the rows beside it, the range
status word, and that one call writes nowhere but where it is told (tests/arena.py)."""
import ctypes
import os
import tempfile
import warnings

import pytest
import torch

from arena import Arena
from gpu_support import dev, g, same_bits
from run_args import nvs_args

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "bf16x3", "f16", "bf16"]
PLANES = {"f16x3": 2, "bf16x3": 2, "f16": 1, "bf16": 1}
ELEMENT = {"f16x3": torch.float16, "f16": torch.float16, "bf16x3": torch.bfloat16, "bf16": torch.bfloat16}
HALF = ("f16x3", "f16")
# tests/generic_cases.py's four, the widths that are no multiple of 8 (the ragged packed loader, ldp > K; W / 2 = 50), and the
# reference's network without view directions, with the depth-supervised variant's softplus density
SHAPES = [dict(D=9, W=320, skips=[4], L=10, Lv=4), dict(D=12, W=96, skips=[3, 6, 9], L=5, Lv=2),
          dict(D=8, W=256, skips=[4], L=12, Lv=6), dict(D=9, W=272, skips=[4], L=10, Lv=0),
          dict(D=9, W=100, skips=[4], L=10, Lv=4), dict(D=9, W=100, skips=[4], L=10, Lv=0, softplus=True)]
W100 = 4
R, S = 21, 37                                        # 777 rows


@pytest.fixture(scope="module")
def P():
    import plnerf_amd
    return plnerf_amd


@pytest.fixture
def generic():
    """HONOUR_PRECISION on for the test (CHAIN_INFERENCE as found: off), both put back afterwards."""
    from plnerf_amd import generic as G
    found = G.HONOUR_PRECISION, G.CHAIN_INFERENCE
    G.HONOUR_PRECISION = True
    try:
        yield G
    finally:
        G.HONOUR_PRECISION, G.CHAIN_INFERENCE = found


def build(P, shape, precision, seed=47):
    D, Wd, skips, Lx, Lv = shape["D"], shape["W"], shape["skips"], shape["L"], shape["Lv"]
    torch.manual_seed(seed)
    emb_fn, in_ch = P.get_embedder(Lx, 0)
    embd_fn, in_ch_v = P.get_embedder(Lv, 0) if Lv > 0 else (None, 0)
    net = P.NeRF(D=D, W=Wd, input_ch=in_ch, input_ch_views=in_ch_v, output_ch=5, skips=skips, use_viewdirs=Lv > 0,
                 precision=precision, density_activation="softplus" if shape.get("softplus") else None).to(dev())
    assert not net.is_supported()
    return net, emb_fn, embd_fn


def embedded_rows(emb_fn, embd_fn, n=R * S):
    """n embedded rows [n, input_ch + view_ch] on the GPU, from seeded points and directions."""
    gen = torch.Generator().manual_seed(53)
    pts = (torch.rand(n, 3, generator=gen) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    cols = [emb_fn(g(pts))] + ([embd_fn(g(vd))] if embd_fn is not None else [])
    return torch.cat(cols, -1).contiguous()


def routes(G, net, rows):
    """(switch off, switch on) under no_grad, each with the status bits it left (the word is cleared in between)."""
    out = []
    for chain in (False, True):
        G.CHAIN_INFERENCE = chain
        with torch.no_grad():
            assert G.chains(net, rows) is chain
            y = G.forward(net, rows)
        out.append((y, net.range_status(reset=True)))
    G.CHAIN_INFERENCE = False
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. pack
def _matrix(rows, K, ld, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, ld, generator=gen) * 3.0
    x[0, :4] = torch.tensor([0.0, -0.0, 65504.0, -65504.0])
    x[rows - 1, K - 3:K] = torch.tensor([65520.0, 1.0e5, -1.0e5])
    return x


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("rows,K,bit", [(37, 63, "RANGE_ACTIVATION"), (5, 100, "RANGE_WEIGHT")])
def test_pack_against_torch(P, precision, rows, K, bit):
    """plnerf_pack_h16 on a matrix whose row stride lies beyond K: hi = x.to(element), lo = (x - hi.float()).to(element) as
    torch computes them on the CPU (both conversions round to nearest even; x - hi is exact in fp32), bitwise; the IEEE-half
    modes clamp 65,520 and +-1e5 to +-65,504 and raise exactly the bit they were handed, the bf16 modes nothing; the columns
    K .. ldp - 1 of a NaN-prefilled destination stay NaN.  Without the three values beyond the range nothing is raised."""
    L = P._lib
    ld, ldp, planes, el = K + 7, L.pack_ld(K), PLANES[precision], ELEMENT[precision]
    assert ldp > K
    for clean in (False, True):
        x = _matrix(rows, K, ld, seed=rows)
        if clean:
            x[rows - 1, K - 3:K] = torch.tensor([65503.0, -3.0e4, 1.0e-7])
        src = g(x)
        dst = torch.full((planes, rows, ldp), -1, dtype=torch.int16, device=dev())      # (0xFFFF: a NaN in both formats)
        status = torch.zeros(1, dtype=torch.int32, device=dev())
        L.check(L.lib().plnerf_pack_h16(L.dptr(src), ld, rows, K, L.PRECISION[precision], ctypes.c_void_p(dst.data_ptr()),
                                        L.dptr(status, "status", torch.int32), getattr(L, bit), L.stream()), "plnerf_pack_h16")
        xk = x[:, :K].clamp(-65504.0, 65504.0) if precision in HALF else x[:, :K]
        hi = xk.to(el)
        want = [hi] + ([(xk - hi.float()).to(el)] if planes == 2 else [])
        got = dst.cpu()
        for plane, ref in enumerate(want):
            assert torch.equal(got[plane, :, :K], ref.view(torch.int16)), (precision, rows, K, plane, clean)
        assert bool((got[:, :, K:] == -1).all())
        assert int(status.item()) == (getattr(L, bit) if precision in HALF and not clean else 0)
    # a NULL status: the clamp is silent
    L.check(L.lib().plnerf_pack_h16(L.dptr(src), ld, rows, K, L.PRECISION[precision], ctypes.c_void_p(dst.data_ptr()), None,
                                    getattr(L, bit), L.stream()), "plnerf_pack_h16")
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------- 2. bit-identity
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=lambda k: "D{D}W{W}L{L}v{Lv}".format(**SHAPES[k]))
def test_one_call_is_the_layered_route_bit_for_bit(P, generic, k, precision):
    net, emb_fn, embd_fn = build(P, SHAPES[k], precision)
    rows = embedded_rows(emb_fn, embd_fn)
    (off, bits_off), (on, bits_on) = routes(generic, net, rows)
    assert off.shape == on.shape == (R * S, 4 if SHAPES[k]["Lv"] > 0 else 5)
    assert bool(torch.isfinite(off).all())
    assert same_bits(on, off), (precision, SHAPES[k], float((on - off).abs().max()))
    assert bits_off == 0 and bits_on == 0
    assert net.__dict__["_chain_workspace"].numel() >= _query(P, net, R * S)


# ------------------------------------------------------------------------------------------------------ the C entry itself
def _shape_of(P, net):
    L = P._lib
    live = sorted(set(s for s in net.skips if 0 <= s < net.D))
    shape = L.GenericShape(D=net.D, W=net.W, input_ch=net.input_ch, view_ch=net.view_ch, use_viewdirs=int(net.use_viewdirs),
                           output_ch=0 if net.use_viewdirs else net.output_linear.out_features,
                           n_view_layers=len(net.views_linears), n_skips=len(live))
    for q, s in enumerate(live):
        shape.skips[q] = s
    return shape


def _query(P, net, n):
    L = P._lib
    return L.lib().plnerf_generic_fwd_workspace_bytes(ctypes.byref(_shape_of(P, net)), n, L.PRECISION[net.precision])


def c_forward(P, net, rows, status=None):
    """plnerf_generic_fwd on `rows` (a 2-D fp32 view whose rows are contiguous; any row stride) with a fresh workspace of
    exactly the queried size: the raw output [n, 4 or output_ch]."""
    L = P._lib
    n = rows.shape[0]
    tensors = list(net.state_dict().values())
    params = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    ws = torch.empty(max(_query(P, net, n), 16), dtype=torch.uint8, device=dev())
    out = torch.full((n, 4 if net.use_viewdirs else net.output_linear.out_features), float("nan"), device=dev())
    rc = L.lib().plnerf_generic_fwd(ctypes.byref(_shape_of(P, net)), params, ctypes.c_void_p(rows.data_ptr()),
                                    rows.stride(0) if n > 1 else rows.shape[1], n, L.PRECISION[net.precision],
                                    ctypes.c_void_p(ws.data_ptr()), _query(P, net, n), ctypes.c_void_p(out.data_ptr()),
                                    out.stride(0), None if status is None else ctypes.c_void_p(status.data_ptr()), L.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------- 3. rows
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_row_does_not_depend_on_the_rows_beside_it(P, precision):
    """W = 320 through the C entry, n = 1, 127, 129, 300: one call on contiguous rows == two calls split at row 131 (n / 2
    where n is shorter) == the same rows at an offset inside a wider, longer array; and a call repeated gives the same bits."""
    net, emb_fn, embd_fn = build(P, SHAPES[0], precision)
    width = net.input_ch + net.view_ch
    big = torch.full((400, width + 5), float("nan"), device=dev())
    big[:, :width] = embedded_rows(emb_fn, embd_fn, 400)
    whole = None
    for n in (1, 127, 129, 300):
        inside = big[7:7 + n, :width]
        assert inside.stride(0) == width + 5
        rows = inside.contiguous()
        one = c_forward(P, net, rows)
        assert bool(torch.isfinite(one).all())
        assert same_bits(c_forward(P, net, rows), one)
        cut = 131 if n > 131 else n // 2
        assert same_bits(torch.cat([c_forward(P, net, rows[:cut]), c_forward(P, net, rows[cut:])]), one), (precision, n)
        assert same_bits(c_forward(P, net, inside), one), (precision, n)
        whole = one if n == 300 else whole
        if n == 300:      # (and the shorter calls were prefixes of this one)
            assert same_bits(c_forward(P, net, rows[:127]), whole[:127])


# --------------------------------------------------------------------------------------------------------------- 4. range
@pytest.mark.parametrize("precision", PRECISIONS)
def test_range_bits_move_from_the_loader_to_the_epilogue(P, generic, precision):
    """A hidden unit beyond 65,504 (pts_linears[1].bias[0] = 1e5): layer 1's epilogue clamps it where layer 2's loader did --
    the same output bits, PLNERF_RANGE_ACTIVATION and only that in the IEEE-half modes, nothing in the bf16 modes.  The same
    with one weight at 1e5 (rgb_linear's, whose result no loader reads: PLNERF_RANGE_WEIGHT alone) and with one +inf among
    the input rows (the first layer's loader, in both routes).  A NULL status is PLNERF_OK."""
    L = P._lib
    half = precision in HALF
    for case, bit in (("bias", L.RANGE_ACTIVATION), ("weight", L.RANGE_WEIGHT), ("inf", L.RANGE_ACTIVATION)):
        net, emb_fn, embd_fn = build(P, SHAPES[W100], precision)
        rows = embedded_rows(emb_fn, embd_fn, 300)
        with torch.no_grad():
            if case == "bias":
                net.pts_linears[1].bias[0] = 1.0e5
            elif case == "weight":
                net.rgb_linear.weight[1, 7] = 1.0e5
            else:
                rows[131, 2] = float("inf")
        (off, bits_off), (on, bits_on) = routes(generic, net, rows)
        assert same_bits(on, off), (precision, case)
        assert bits_off == bits_on == (bit if half else 0), (precision, case, bits_off, bits_on)
        if case == "bias":
            assert same_bits(c_forward(P, net, rows, status=None), off)
            word = torch.zeros(1, dtype=torch.int32, device=dev())
            assert same_bits(c_forward(P, net, rows, status=word), off) and int(word.item()) == (bit if half else 0)


# --------------------------------------------------------------------------------------------------------- 5. containment
@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_one_call_writes_only_what_it_is_handed(P, precision):
    """Every buffer of one call carved from a guard-banded arena, at the W = 100 shape with n = 129: the guards intact, the
    inputs unchanged, the padding columns of `out` still NaN, every written element finite -- with the workspace (exactly the
    queried size; no initialisation required) once at 0x00 and once at 0xFF, both giving the same bits."""
    L = P._lib
    net, emb_fn, embd_fn = build(P, SHAPES[W100], precision)
    n, width, ld_rows, ld_out = 129, net.input_ch + net.view_ch, net.input_ch + net.view_ch + 3, 4 + 3
    tensors = list(net.state_dict().values())
    need = _query(P, net, n)
    sizes = [n * ld_rows * 4, need, n * ld_out * 4, 4] + [t.numel() * 4 for t in tensors]
    results = []
    for fill in (0x00, 0xFF):
        arena = Arena(dev(), sum(Arena.room(b) for b in sizes) + (1 << 20))
        rows_b = arena.carve("rows", n * ld_rows * 4, align=4, role="in")
        rows_b.f32().view(n, ld_rows)[:, :width] = embedded_rows(emb_fn, embd_fn, n)
        rows_b.freeze()
        param_b = []
        for q, t in enumerate(tensors):
            b = arena.carve(f"param{q}", t.numel() * 4, align=4, role="in")
            b.put(t.detach())
            b.freeze()
            param_b.append(b)
        ws = arena.carve("workspace", need, align=L.GENERIC_WORKSPACE_ALIGN, role="scratch")
        ws.set_bytes(fill)
        out_b = arena.carve("out", n * ld_out * 4, align=4, role="out")
        status = arena.carve("status", 4, align=4, role="zeroed")
        params = (ctypes.c_void_p * len(param_b))(*[b.dptr for b in param_b])
        rc = L.lib().plnerf_generic_fwd(ctypes.byref(_shape_of(P, net)), params, ctypes.c_void_p(rows_b.dptr), ld_rows, n,
                                        L.PRECISION[precision], ctypes.c_void_p(ws.dptr), need, ctypes.c_void_p(out_b.dptr), ld_out,
                                        ctypes.c_void_p(status.dptr), L.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        arena.check()
        out = out_b.f32().view(n, ld_out)
        assert bool(torch.isnan(out[:, 4:]).all()) and bool(torch.isfinite(out[:, :4]).all())
        results.append(out[:, :4].clone())
    assert same_bits(results[0], results[1])
    assert same_bits(results[0], c_forward(P, net, embedded_rows(emb_fn, embd_fn, n)))


# ----------------------------------------------------------------------------------------------------------- 6. grad mode
@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_under_grad_mode_the_layered_route_runs_as_before(P, generic, precision):
    net, emb_fn, embd_fn = build(P, SHAPES[1], precision)
    rows = embedded_rows(emb_fn, embd_fn)
    cot = g(torch.randn(R * S, 4, generator=torch.Generator().manual_seed(59)))

    def run(chain):
        generic.CHAIN_INFERENCE = chain
        net.zero_grad()
        assert not generic.chains(net, rows)
        out = generic.forward(net, rows)
        assert out.requires_grad
        (out * cot).sum().backward()
        return out.detach(), [p.grad.clone() for p in net.parameters() if p.grad is not None]
    off, grads_off = run(False)
    on, grads_on = run(True)
    assert same_bits(on, off) and len(grads_on) == len(grads_off) > 0
    assert all(same_bits(a, b) for a, b in zip(grads_on, grads_off))
    # frozen parameters and rows without a gradient: nothing to record, so the one-call entry serves grad mode too
    for p in net.parameters():
        p.requires_grad_(False)
    assert generic.chains(net, rows) and not generic.chains(net, rows.clone().requires_grad_(True))
    assert same_bits(generic.forward(net, rows), off)
    assert net.range_status() == 0


# ------------------------------------------------------------------------------------------------------------ 7. render()
def test_render_of_a_small_view(P, generic):
    """24 x 16 pixels at 16 + 16 samples through create_nerf's W = 320 pair in f16x3, rendered with render_kwargs_test: every
    map the switch-on render returns has the bits of the switch-off render's, and create_nerf says which route runs."""
    H, W = 16, 24

    def nets(chain):
        generic.CHAIN_INFERENCE = chain
        d = tempfile.mkdtemp()
        os.makedirs(os.path.join(d, "exp"))
        args = nvs_args(d, "f16x3", N_rand=64, netwidth=320, netwidth_fine=320, N_samples=16, N_importance=16)
        torch.manual_seed(5)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _, kw_test, _, _, _, _ = P.create_nerf(args, device=dev())
        told = [str(w.message) for w in caught if "layer by layer" in str(w.message)]
        assert len(told) == 2 and all(("plnerf_generic_fwd" in m) is chain and "a no-grad forward takes" in m for m in told), told
        return kw_test
    nets(False)
    kw = nets(True)
    assert not kw["network_fn"].is_supported() and not kw["network_fine"].is_supported()
    K = [[1.3 * W, 0, W / 2], [0, 1.3 * W, H / 2], [0, 0, 1]]
    c2w = g(P.rays.pose_spherical(40.0, -25.0, 4.0)[:3, :4])

    def run(chain):
        generic.CHAIN_INFERENCE = chain
        torch.manual_seed(71)      # (render_kwargs_test perturbs, as the reference's does: the same torch.rand draws in both)
        with torch.no_grad():
            rgb, disp, acc, extras = P.render(H, W, K, chunk=32768, c2w=c2w, near=2.0, far=6.0, **kw)
        return dict({k: v for k, v in extras.items() if torch.is_tensor(v)}, rgb_map=rgb, disp_map=disp, acc_map=acc)
    on, off = run(True), run(False)
    assert set(on) == set(off) and {"rgb_map", "rgb0", "acc0"} <= set(on)
    for name in sorted(on):
        assert same_bits(on[name], off[name]), name
    assert float(off["acc_map"].max()) > 0.0      # (the view met density: the networks did run)
    assert kw["network_fn"].range_status() == 0 and kw["network_fine"].range_status() == 0
    assert "_chain_workspace" in kw["network_fn"].__dict__ and "_chain_workspace" in kw["network_fine"].__dict__
