"""generic.HONOUR_PRECISION_BACKWARD: networks outside the compiled trunk with forward AND backward in the network's own 16-bit
mode (plnerf_gemm_h16, plnerf_gemm_h16_dgrad / _wgrad) -- the gradients through run_network against the same module in fp64
torch, the switch against the forward switch alone, and one guarded training step."""
import os
import tempfile
import warnings

import pytest
import torch

import generic_cases as C
from gpu_support import counting_calls, dev, g, same_bits
from run_args import nvs_args

pytestmark = pytest.mark.gpu

BACKWARD_ENTRIES = {"plnerf_gemm_h16_dgrad", "plnerf_gemm_h16_wgrad"}


@pytest.fixture(scope="module")
def P():
    import plnerf_amd
    return plnerf_amd


@pytest.fixture
def both():
    """Both switches on for the test, put back afterwards."""
    from plnerf_amd import generic
    found = generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD
    generic.HONOUR_PRECISION = generic.HONOUR_PRECISION_BACKWARD = True
    try:
        yield generic
    finally:
        generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD = found


def forward_recording(P, net, emb_fn, embd_fn, pts, vd):
    """run_network's output and, per ReLU layer in the route's order, the branch the GPU's forward took."""
    from plnerf_amd import generic
    taken, found = [], generic.linear

    def recording(x, layer, relu, *rest):
        y = found(x, layer, relu, *rest)
        if relu:
            taken.append(y.detach() > 0)
        return y
    generic.linear = recording
    try:
        out = P.run_network(g(pts), g(vd) if embd_fn is not None else None, net, emb_fn, embd_fn)
    finally:
        generic.linear = found
    return out, taken


def worst_gradient_error(net, leaves, scale=1.0):
    """max over the parameters of |grad - scale * fp64 grad| / max |scale * fp64 grad|."""
    worst = 0.0
    for name, prm in net.named_parameters():
        r = leaves[name].grad
        if r is None:      # (views_linears without view directions: not on the path, as in the reference)
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0
            continue
        assert bool(torch.isfinite(prm.grad).all()), name
        r = r * scale
        worst = max(worst, float((prm.grad.cpu().double() - r).abs().max()) / max(float(r.abs().max()), 1e-9 * scale))
    return worst


def fp64_gradients(P, k, cot, branches=None):
    sd, forward, _, _ = C.reference(P, k)
    leaves = {n: t.clone().requires_grad_(True) for n, t in sd.items()}
    (forward(leaves, branches)[0][:, :4] * cot.reshape(-1, 4).double()).sum().backward()
    return leaves


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3", "f16", "bf16"])
@pytest.mark.parametrize("k", range(len(C.SHAPES)), ids=lambda k: "D{D}W{W}L{L}v{Lv}".format(**C.SHAPES[k]))
def test_gradients_in_their_own_precision_against_fp64(P, both, k, precision):
    """Both switches on, through run_network, the shapes, 777 rows, seeds and inputs of tests/test_gpu_generic_precision.py.
    The backward's gate is the activation the 16-bit forward wrote, so -- that file's rule -- a unit (of one row) whose fp64
    pre-activation lies inside the mode's forward error is undecided: there the fp64 reference's backward takes the branch
    the GPU's forward took, everywhere else its own; the share of such units is capped at 1 % per layer, asserted on the
    fp64 pre-activations.  x3 modes: every parameter's gradient within 2e-4 of max |g|.  Plain modes: gradients finite, the
    status word 0, the worst error (against the fp64 reference on its own branches) printed.  Every layer's backward ran on
    the 16-bit entries and none on plnerf_gemm_f32."""
    shape = C.SHAPES[k]
    sd, forward, ref, pre = C.reference(P, k)
    net, emb_fn, embd_fn = C.build(P, shape, precision)
    pts, vd, cot = C.inputs()
    split = precision in C.FLIP_BELOW
    out, taken = forward_recording(P, net, emb_fn, embd_fn, pts, vd)
    with counting_calls() as lib:
        (out[..., :4] * g(cot)).sum().backward()
    torch.cuda.synchronize()
    assert set(lib.calls) == BACKWARD_ENTRIES, set(lib.calls)
    assert net.range_status() == 0
    if not split:
        worst = worst_gradient_error(net, fp64_gradients(P, k, cot))
        print(f"{precision} {shape}: worst gradient error / max |g| {worst:.2e} (printed, not bounded here)")
        return
    undecided = [z.abs() < C.FLIP_BELOW[precision] for z in pre]
    shares = [float(u.double().mean()) for u in undecided]
    assert len(taken) == len(pre) and max(shares) <= 0.01, shares
    branches = [torch.where(u, t.cpu(), z > 0) for u, t, z in zip(undecided, taken, pre)]
    worst = worst_gradient_error(net, fp64_gradients(P, k, cot, branches))
    print(f"{precision} {shape}: worst gradient error / max |g| {worst:.2e}; undecided units per layer max {max(shares):.2e}")
    assert worst <= C.GRAD_TOL, (precision, shape, worst)


@pytest.mark.parametrize("scale", [1e-12, 1e12])
def test_gradients_of_a_scaled_cotangent(P, both, scale):
    """f16x3, D = 9, W = 320: the cotangent times 1e-12 (far below the half range) and times 1e12 -- the same 2e-4 of
    max |g|: the launch scale carries the gradient into the half range, and no range bit is set."""
    k, precision = 0, "f16x3"
    sd, forward, ref, pre = C.reference(P, k)
    net, emb_fn, embd_fn = C.build(P, C.SHAPES[k], precision)
    pts, vd, cot = C.inputs()
    out, taken = forward_recording(P, net, emb_fn, embd_fn, pts, vd)
    (out[..., :4] * g(cot * scale)).sum().backward()
    torch.cuda.synchronize()
    assert net.range_status() == 0
    undecided = [z.abs() < C.FLIP_BELOW[precision] for z in pre]
    branches = [torch.where(u, t.cpu(), z > 0) for u, t, z in zip(undecided, taken, pre)]
    worst = worst_gradient_error(net, fp64_gradients(P, k, cot, branches), float(torch.tensor(scale, dtype=torch.float32)))
    print(f"{precision} cotangent x {scale:g}: worst gradient error / max |g| {worst:.2e}")
    assert worst <= C.GRAD_TOL, (scale, worst)


def test_the_switch(P):
    """D = 9, W = 320 in f16 (the plain mode: a 16-bit backward is visibly not the fp32 one).  Off is the default: with the
    forward switch alone the backward issues plnerf_gemm_f32 products only, as before.  Backward switch on: the forward is
    bit-identical to the forward switch alone, the backward issues the two 16-bit entries only, and the gradients differ
    somewhere from the fp32-backward ones; switched off again they are the first run's, bit for bit.  The backward switch
    WITHOUT the forward switch changes nothing (bit for bit the route with both off), and an fp32 network ignores both."""
    from plnerf_amd import generic
    assert generic.HONOUR_PRECISION is False and generic.HONOUR_PRECISION_BACKWARD is False
    shape = C.SHAPES[0]
    pts, vd, cot = C.inputs()
    net16, emb_fn, embd_fn = C.build(P, shape, "f16")
    net32, _, _ = C.build(P, shape, "fp32")
    net32.load_state_dict(net16.state_dict())

    def run(net, forward_switch, backward_switch):
        generic.HONOUR_PRECISION, generic.HONOUR_PRECISION_BACKWARD = forward_switch, backward_switch
        try:
            net.zero_grad()
            out = P.run_network(g(pts), g(vd), net, emb_fn, embd_fn)
            with counting_calls() as lib:
                (out[..., :4] * g(cot)).sum().backward()
            return out.detach(), [p.grad.clone() for p in net.parameters()], set(lib.calls)
        finally:
            generic.HONOUR_PRECISION = generic.HONOUR_PRECISION_BACKWARD = False

    def equal(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))
    out_off, grads_off, calls_off = run(net16, False, False)
    out_fwd, grads_fwd, calls_fwd = run(net16, True, False)
    out_both, grads_both, calls_both = run(net16, True, True)
    assert calls_off == calls_fwd == {"plnerf_gemm_f32"} and calls_both == BACKWARD_ENTRIES
    assert same_bits(out_both, out_fwd) and not same_bits(out_fwd, out_off)
    assert not equal(grads_both, grads_fwd)
    again_out, again_grads, _ = run(net16, True, False)
    assert same_bits(again_out, out_fwd) and equal(again_grads, grads_fwd)
    # the backward switch alone: nothing changes
    out_bwd, grads_bwd, calls_bwd = run(net16, False, True)
    assert same_bits(out_bwd, out_off) and equal(grads_bwd, grads_off) and calls_bwd == {"plnerf_gemm_f32"}
    # an fp32 network ignores both
    out32, grads32, _ = run(net32, False, False)
    on32, on_grads32, calls32 = run(net32, True, True)
    assert same_bits(on32, out32) and equal(on_grads32, grads32) and calls32 == {"plnerf_gemm_f32"}
    assert same_bits(out32, out_off) and equal(grads32, grads_off)


def _train_step(P, precision):
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "exp"))
    args = nvs_args(d, precision, N_rand=64, netwidth=320, netwidth_fine=320, N_samples=16, N_importance=16)
    torch.manual_seed(5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        kw, _, start, _, opt, opt_c = P.create_nerf(args, device=dev())
    told = [str(w.message) for w in caught if "layer by layer" in str(w.message)]
    named = f"the backward in precision={precision!r} (plnerf_gemm_h16_dgrad / _wgrad)"
    assert len(told) == 2 and all(f"the forward in precision={precision!r} (plnerf_gemm_h16)" in m and named in m and
                                  "backward in fp32" not in m for m in told), told
    ts = P.TrainStep(args, kw, opt, opt_c, start=start, distributed=False, seed=3, range_check_every=0)
    return ts, kw, opt, opt_c


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_one_guarded_training_step(P, both, precision):
    """create_nerf with netwidth 320, 64 rays, 16 + 16 samples, both switches on: the warning names the 16-bit backward, the
    step runs its backward on the 16-bit entries, applies, the loss is finite, both status words are 0 and no step is
    withheld."""
    ts, kw, opt, opt_c = _train_step(P, precision)
    coarse, fine = kw["network_fn"], kw["network_fine"]
    assert not coarse.is_supported() and not fine.is_supported()
    before = [p.detach().clone() for n in (coarse, fine) for p in n.parameters()]
    H, W = 20, 26
    gen = torch.Generator().manual_seed(11)
    image = g(torch.rand(H, W, 3, generator=gen))
    K = [[1.3 * W, 0, W / 2], [0, 1.3 * W, H / 2], [0, 0, 1]]
    c2w = P.rays.pose_spherical(30.0, -30.0, 4.0)
    with counting_calls() as lib:
        loss, _ = ts.step_view(H, W, K, c2w, image, near=2.0, far=6.0, n_rand=64)
    torch.cuda.synchronize()
    assert BACKWARD_ENTRIES <= set(lib.calls) and "plnerf_gemm_f32" not in lib.calls and "plnerf_gemm_h16" in lib.calls
    after = [p.detach() for n in (coarse, fine) for p in n.parameters()]
    assert bool(torch.isfinite(loss))
    assert coarse.range_status() == 0 and fine.range_status() == 0
    ts.check_range()
    assert opt.withheld_steps() == 0 and opt_c.withheld_steps() == 0
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    assert all(bool(torch.isfinite(a).all()) for a in after)
