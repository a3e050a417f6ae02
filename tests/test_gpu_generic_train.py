"""generic.CHAIN_TRAINING and include/experimental/plnerf_hip_generic_train.h: a training forward and backward of the
layer-by-layer route as one library call each.  The oracle everywhere is the route it replaces -- the layered route with
generic.HONOUR_PRECISION and generic.HONOUR_PRECISION_BACKWARD both on (tests/test_gpu_generic_backward.py holds that route to
fp64) -- BIT FOR BIT: the outputs, every parameter's .grad and the range status word, which is cleared between the routes.
The upstream gradient is a seeded weighting of the outputs of magnitude ~1e-6, so that the IEEE-half modes need their scale."""
import ctypes

import pytest
import torch

from arena import Arena
from gpu_support import dev, g, same_bits

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "bf16x3", "f16", "bf16"]
HALF = ("f16x3", "f16")
# tests/test_gpu_generic_chain.py's six, restated (no test module imports another): ragged widths (100, 272, W / 2 = 50), three
# skips, no view directions, the depth-supervised variant's softplus density
SHAPES = [dict(D=9, W=320, skips=[4], L=10, Lv=4), dict(D=12, W=96, skips=[3, 6, 9], L=5, Lv=2),
          dict(D=8, W=256, skips=[4], L=12, Lv=6), dict(D=9, W=272, skips=[4], L=10, Lv=0),
          dict(D=9, W=100, skips=[4], L=10, Lv=4), dict(D=9, W=100, skips=[4], L=10, Lv=0, softplus=True)]
W320, W100 = 0, 4
# the containment test's (small enough to map onto the compiled trunk, which Python would route it to: the C entries take any shape)
SMALL = dict(D=3, W=100, skips=[1], L=10, Lv=4)
R, S = 21, 37                                        # 777 rows
IDS = dict(ids=lambda k: "D{D}W{W}L{L}v{Lv}".format(**SHAPES[k]))


@pytest.fixture(scope="module")
def P():
    import plnerf_amd
    return plnerf_amd


@pytest.fixture
def generic(monkeypatch):
    """Both opt-ins of the layered 16-bit route on for the test (CHAIN_TRAINING and CHAIN_INFERENCE as found: off), all put
    back afterwards; G.layered counts the layers that went through the layered route's LinearFn."""
    from plnerf_amd import generic as G
    found = G.HONOUR_PRECISION, G.HONOUR_PRECISION_BACKWARD, G.CHAIN_INFERENCE, G.CHAIN_TRAINING
    G.HONOUR_PRECISION = G.HONOUR_PRECISION_BACKWARD = True
    linear, calls = G.linear, []

    def counted(*args, **kwargs):
        calls.append(1)
        return linear(*args, **kwargs)
    monkeypatch.setattr(G, "linear", counted)
    G.layered = calls
    try:
        yield G
    finally:
        G.HONOUR_PRECISION, G.HONOUR_PRECISION_BACKWARD, G.CHAIN_INFERENCE, G.CHAIN_TRAINING = found
        del G.layered


def build(P, shape, precision, seed=47, outside_trunk=True):
    D, Wd, skips, Lx, Lv = shape["D"], shape["W"], shape["skips"], shape["L"], shape["Lv"]
    torch.manual_seed(seed)
    emb_fn, in_ch = P.get_embedder(Lx, 0)
    embd_fn, in_ch_v = P.get_embedder(Lv, 0) if Lv > 0 else (None, 0)
    net = P.NeRF(D=D, W=Wd, input_ch=in_ch, input_ch_views=in_ch_v, output_ch=5, skips=skips, use_viewdirs=Lv > 0,
                 precision=precision, density_activation="softplus" if shape.get("softplus") else None).to(dev())
    assert net.is_supported() is not outside_trunk
    return net, emb_fn, embd_fn


def embedded_rows(emb_fn, embd_fn, n=R * S):
    """n embedded rows [n, input_ch + view_ch] on the GPU, from seeded points and directions."""
    gen = torch.Generator().manual_seed(53)
    pts = (torch.rand(n, 3, generator=gen) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    cols = [emb_fn(g(pts))] + ([embd_fn(g(vd))] if embd_fn is not None else [])
    return torch.cat(cols, -1).contiguous()


def weights_of(n, cols, seed=59):
    """The loss is (out * weights).sum(): its gradient with respect to `out` is `weights`, ~1e-6."""
    return g(torch.randn(n, cols, generator=torch.Generator().manual_seed(seed)) * 1.0e-6)


def step(G, net, chunks, weights, chain, expect=None):
    """One forward per chunk and one backward of the summed loss with the switch at `chain`: (outputs, {name: grad or None},
    status bits); the word is left cleared.  expect: what chains_training must say (default: `chain`)."""
    G.CHAIN_TRAINING = chain
    net.zero_grad(set_to_none=True)
    del G.layered[:]
    outs, loss = [], 0.0
    for rows, w in zip(chunks, weights):
        assert G.chains_training(net, rows) is (chain if expect is None else expect)
        out = G.forward(net, rows)
        assert out.requires_grad
        outs.append(out)
        loss = loss + (out * w).sum()
    loss.backward()
    G.CHAIN_TRAINING = False
    grads = {name: None if p.grad is None else p.grad.clone() for name, p in net.named_parameters()}
    return [o.detach() for o in outs], grads, net.range_status(reset=True) if G.honours(net) else 0


def assert_same_step(on, off, what):
    (outs_on, grads_on, bits_on), (outs_off, grads_off, bits_off) = on, off
    for a, b in zip(outs_on, outs_off):
        assert a.shape == b.shape and same_bits(a, b), (what, "out", float((a - b).abs().max()))
    assert set(grads_on) == set(grads_off)
    for name in grads_off:
        a, b = grads_on[name], grads_off[name]
        assert (a is None) == (b is None), (what, name)
        if b is not None:
            assert a.shape == b.shape and same_bits(a, b), (what, name, float((a - b).abs().max()), float(b.abs().max()))
    assert bits_on == bits_off, (what, bits_on, bits_off)


def both(G, net, chunks, weights, what):
    """The layered oracle, then the one-call route, compared bit for bit; the oracle's step is returned."""
    off = step(G, net, chunks, weights, False)
    assert len(G.layered) > 0
    on = step(G, net, chunks, weights, True)
    assert len(G.layered) == 0, "the layered LinearFn was entered"
    assert_same_step(on, off, what)
    return off


# ------------------------------------------------------------------------------------------------------------ 1. equality
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", range(len(SHAPES)), **IDS)
def test_one_call_each_way_is_the_layered_route_bit_for_bit(P, generic, k, precision):
    net, emb_fn, embd_fn = build(P, SHAPES[k], precision)
    rows = embedded_rows(emb_fn, embd_fn)
    cols = 4 if SHAPES[k]["Lv"] > 0 else 5
    outs, grads, bits = both(generic, net, [rows], [weights_of(R * S, cols)], (precision, SHAPES[k]))
    assert outs[0].shape == (R * S, cols) and bool(torch.isfinite(outs[0]).all()) and bits == 0
    took_part = [name for name, v in grads.items() if v is not None]
    assert len(took_part) == 2 * (SHAPES[k]["D"] + (4 if SHAPES[k]["Lv"] > 0 else 1))      # (without view directions: no view layer)
    assert all(float(grads[name].abs().max()) > 0.0 for name in took_part if name.endswith("weight"))


# ------------------------------------------------------------------------------------------------------- 2. split wgrad
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [W100, W320], **IDS)
def test_the_split_weight_gradient(P, generic, k, precision):
    """1,600 rows: the smallest size at which the hidden layers' weight gradients are dealt over three splits whose last is
    ragged (50 stages: 17 + 17 + 16, i.e. 544 + 544 + 512 rows), summed in split order."""
    W = SHAPES[k]["W"]
    assert generic._splits(W, W + 1, 1600) == 3 and -(-1600 // 32) == 50
    net, emb_fn, embd_fn = build(P, SHAPES[k], precision)
    rows = embedded_rows(emb_fn, embd_fn, 1600)
    both(generic, net, [rows], [weights_of(1600, 4)], (precision, SHAPES[k], 1600))


# -------------------------------------------------------------------------------------------------------- 3. two chunks
@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_chunks_and_one_backward(P, generic, precision):
    """The network called on rows [0, 1000) and [1000, 1600) in one graph, then one backward: each call's saved state is its
    own (run_network calls a network once per netchunk before any backward runs)."""
    net, emb_fn, embd_fn = build(P, SHAPES[W100], precision)
    rows, w = embedded_rows(emb_fn, embd_fn, 1600), weights_of(1600, 4)
    both(generic, net, [rows[:1000], rows[1000:]], [w[:1000], w[1000:]], (precision, "two chunks"))


# ------------------------------------------------------------------------------------------------------------- 4. the gate
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_the_gate_below_the_half_range(P, generic, precision):
    """Three units of layer 0 with zero weights and biases 1e-9, -1e-9, 0: the first one's output is positive but packs to
    hi = lo = 0 in IEEE half, and the layered backward still lets its gradient through -- so must the saved gate plane."""
    net, emb_fn, embd_fn = build(P, SHAPES[W100], precision)
    units = [5, 38, 71]
    with torch.no_grad():
        net.pts_linears[0].weight[units] = 0.0
        net.pts_linears[0].bias[units] = g(torch.tensor([1.0e-9, -1.0e-9, 0.0]))
    rows = embedded_rows(emb_fn, embd_fn)
    if precision == "f16x3":
        assert float(torch.tensor(1.0e-9).half()) == 0.0      # (hi = 0, hence lo = half(1e-9 - 0) = 0 too)
    outs, grads, bits = both(generic, net, [rows], [weights_of(R * S, 4)], (precision, "gate"))
    db = grads["pts_linears.0.bias"][units].tolist()
    assert db[0] != 0.0 and db[1] == 0.0 and db[2] == 0.0, db
    assert bits == 0


# ------------------------------------------------------------------------------------------------------------- 5. the range
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", ["clean", "weight", "input", "inf_gradient"])
def test_range_status(P, generic, precision, case):
    """Equal words and equal gradients: nothing raised on a clean network; PLNERF_RANGE_WEIGHT for a weight of 1e5,
    PLNERF_RANGE_ACTIVATION for an input element of 1e5 and for an infinite upstream gradient (max |g| not finite: s = 0, the
    gradient clamped) in the IEEE-half modes; nothing at all in the bf16 modes."""
    L = P._lib
    net, emb_fn, embd_fn = build(P, SHAPES[W100], precision)
    rows, w = embedded_rows(emb_fn, embd_fn, 300), weights_of(300, 4)
    with torch.no_grad():
        if case == "weight":
            net.rgb_linear.weight[1, 7] = 1.0e5
        elif case == "input":
            rows[131, 2] = 1.0e5
        elif case == "inf_gradient":
            w[77, 1] = float("inf")
    _, grads, bits = both(generic, net, [rows], [w], (precision, case))
    want = {"clean": 0, "weight": L.RANGE_WEIGHT, "input": L.RANGE_ACTIVATION, "inf_gradient": L.RANGE_ACTIVATION}[case]
    if precision not in HALF or case == "clean":
        assert bits == 0, (precision, case, bits)
    else:
        assert bits & want == want, (precision, case, bits)
    if case == "clean":
        assert all(bool(torch.isfinite(v).all()) for v in grads.values() if v is not None)


# --------------------------------------------------------------------------------------------------------- 6. the fallbacks
def test_what_the_switch_leaves_to_the_layered_route(P, generic):
    G = generic
    net, emb_fn, embd_fn = build(P, SHAPES[W100], "f16x3")
    rows, w = embedded_rows(emb_fn, embd_fn, 300), weights_of(300, 4)
    off = step(G, net, [rows], [w], False)

    # rows that require grad (pose or input gradients)
    wanted = rows.clone().requires_grad_(True)
    on = step(G, net, [wanted], [w], True, expect=False)
    assert len(G.layered) > 0 and wanted.grad is not None
    assert_same_step(on, off, "rows.requires_grad")
    # the 16-bit backward switched off: the chain's backward is 16-bit, so it does not apply
    G.HONOUR_PRECISION_BACKWARD = False
    fp32_backward = step(G, net, [rows], [w], False)
    on = step(G, net, [rows], [w], True, expect=False)
    assert len(G.layered) > 0
    assert_same_step(on, fp32_backward, "HONOUR_PRECISION_BACKWARD off")
    G.HONOUR_PRECISION_BACKWARD = True
    # no_grad with CHAIN_INFERENCE: the inference chain, as before
    G.CHAIN_INFERENCE = G.CHAIN_TRAINING = True
    with torch.no_grad():
        assert G.chains(net, rows) and not G.chains_training(net, rows)
        del G.layered[:]
        assert same_bits(G.forward(net, rows), off[0][0]) and len(G.layered) == 0
    G.CHAIN_INFERENCE = G.CHAIN_TRAINING = False
    assert net.range_status(reset=True) == 0

    # an fp32 network
    net, emb_fn, embd_fn = build(P, SHAPES[W100], "fp32")
    off = step(G, net, [rows], [w], False)
    on = step(G, net, [rows], [w], True, expect=False)
    assert len(G.layered) > 0
    assert_same_step(on, off, "fp32")

    # more than PLNERF_GENERIC_MAX_SKIPS live skips
    deep = dict(D=19, W=32, skips=list(range(17)), L=4, Lv=2)
    net, emb_fn, embd_fn = build(P, deep, "bf16x3")
    rows, w = embedded_rows(emb_fn, embd_fn, 130), weights_of(130, 4)
    off = step(G, net, [rows], [w], False)
    on = step(G, net, [rows], [w], True, expect=False)
    assert len(G.layered) > 0
    assert_same_step(on, off, "17 live skips")


# -------------------------------------------------------------------------------------------------------- 7. containment
def _shape_of(P, net):
    L = P._lib
    live = sorted(set(s for s in net.skips if 0 <= s < net.D))
    shape = L.GenericShape(D=net.D, W=net.W, input_ch=net.input_ch, view_ch=net.view_ch, use_viewdirs=int(net.use_viewdirs),
                           output_ch=0 if net.use_viewdirs else net.output_linear.out_features,
                           n_view_layers=len(net.views_linears), n_skips=len(live))
    for q, s in enumerate(live):
        shape.skips[q] = s
    return shape


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_the_raw_entries_write_only_what_they_are_handed(P, precision):
    """D = 3, W = 100, one skip, 37 rows through the C entries, every buffer carved from a guard-banded arena: the guards
    intact, the inputs (rows, parameters, the upstream gradient; `saved` during the backward) unchanged, the padding columns of
    `out` still NaN; `out` is plnerf_generic_fwd's bit for bit; a second, identical backward gives the same bits; and with
    `saved` and the workspace (exactly the queried sizes; no initialisation required) at 0x00 and at 0xFF the same bits."""
    L = P._lib
    lib = L.lib()
    net, emb_fn, embd_fn = build(P, SMALL, precision, outside_trunk=False)
    n, width, code = 37, net.input_ch + net.view_ch, L.PRECISION[precision]
    ld_rows, ld_out, ld_g = width + 3, 4 + 3, 4 + 1
    shape = _shape_of(P, net)
    tensors = list(net.state_dict().values())
    dims = [tuple(t.shape) for t in tensors[0::2]]
    need_s = lib.plnerf_generic_train_saved_bytes(ctypes.byref(shape), n, code)
    need_w = lib.plnerf_generic_train_workspace_bytes(ctypes.byref(shape), n, code)
    need_f = lib.plnerf_generic_fwd_workspace_bytes(ctypes.byref(shape), n, code)
    assert need_s > 0 and need_w > 0 and need_f > 0
    sizes = [n * ld_rows * 4, need_s, need_w, need_f, n * ld_out * 4, n * ld_out * 4, n * ld_g * 4, 4] + \
            [t.numel() * 4 for t in tensors] + [N * (K + 1) * 4 for N, K in dims]
    results = []
    for fill in (0x00, 0xFF):
        arena = Arena(dev(), sum(Arena.room(b) for b in sizes) + (1 << 20))
        rows_b = arena.carve("rows", n * ld_rows * 4, align=4, role="in")
        rows_b.f32().view(n, ld_rows)[:, :width] = embedded_rows(emb_fn, embd_fn, n)
        rows_b.freeze()
        g_b = arena.carve("g_out", n * ld_g * 4, align=4, role="in")
        g_b.f32().view(n, ld_g)[:, :4] = weights_of(n, 4)
        g_b.freeze()
        param_b = []
        for q, t in enumerate(tensors):
            b = arena.carve(f"param{q}", t.numel() * 4, align=4, role="in")
            b.put(t.detach())
            b.freeze()
            param_b.append(b)
        saved = arena.carve("saved", need_s, align=L.GENERIC_WORKSPACE_ALIGN, role="scratch")
        saved.set_bytes(fill)
        ws = arena.carve("workspace", need_w, align=L.GENERIC_WORKSPACE_ALIGN, role="scratch")
        ws.set_bytes(fill)
        ws_f = arena.carve("fwd workspace", need_f, align=L.GENERIC_WORKSPACE_ALIGN, role="scratch")
        out_b = arena.carve("out", n * ld_out * 4, align=4, role="out")
        ref_b = arena.carve("out of plnerf_generic_fwd", n * ld_out * 4, align=4, role="out")
        status = arena.carve("status", 4, align=4, role="zeroed")
        grad_b = [arena.carve(f"grad{q}", N * (K + 1) * 4, align=4, role="out") for q, (N, K) in enumerate(dims)]
        params = (ctypes.c_void_p * len(param_b))(*[b.dptr for b in param_b])
        grads = (ctypes.c_void_p * len(grad_b))(*[b.dptr for b in grad_b])
        p = ctypes.c_void_p
        rc = lib.plnerf_generic_train_fwd(ctypes.byref(shape), params, p(rows_b.dptr), ld_rows, n, code, p(saved.dptr), need_s,
                                          p(out_b.dptr), ld_out, p(status.dptr), L.stream())
        assert rc == 0, rc
        rc = lib.plnerf_generic_fwd(ctypes.byref(shape), params, p(rows_b.dptr), ld_rows, n, code, p(ws_f.dptr), need_f,
                                    p(ref_b.dptr), ld_out, p(status.dptr), L.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        arena.check()
        out, ref = out_b.f32().view(n, ld_out), ref_b.f32().view(n, ld_out)
        assert bool(torch.isnan(out[:, 4:]).all()) and bool(torch.isfinite(out[:, :4]).all())
        assert same_bits(out[:, :4], ref[:, :4])
        saved.freeze()      # (the backward only reads it)
        passes = []
        for again in range(2):
            rc = lib.plnerf_generic_train_bwd(ctypes.byref(shape), p(rows_b.dptr), ld_rows, n, code, p(saved.dptr), need_s,
                                              p(g_b.dptr), ld_g, grads, p(ws.dptr), need_w, p(status.dptr), L.stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            arena.check()
            passes.append([b.f32().clone() for b in grad_b])
        assert all(bool(torch.isfinite(t).all()) for t in passes[0])
        assert all(same_bits(a, b) for a, b in zip(passes[0], passes[1]))
        results.append([out[:, :4].clone()] + passes[0])
    assert all(same_bits(a, b) for a, b in zip(results[0], results[1]))
    assert any(float(t.abs().max()) > 0.0 for t in results[0][1:])
