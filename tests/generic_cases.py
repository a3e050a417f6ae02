"""What the tests of the layer-by-layer route's 16-bit backward (tests/test_gpu_generic_backward.py) take from
tests/test_gpu_generic_precision.py, restated here because no test module imports another: the four network shapes outside
the compiled trunk, the 777 rows, the seeds and inputs, the bounds, and the fp64 reference whose ReLU backward can be told
which branch to take at undecided units."""
import torch

from gpu_support import dev

# tests/test_gpu_modes.py's bounds per mode on the compiled trunk: forward error / (1 + max |reference|)
FORWARD_TOL = {"f16x3": 1e-5, "bf16x3": 3e-5, "f16": 2e-3, "bf16": 1e-2}
FLIP_BELOW = {"f16x3": 1e-5, "bf16x3": 5e-5}      # (the mode's forward error on a hidden unit)
GRAD_TOL = 2e-4                                      # of max |g|
SHAPES = [dict(D=9, W=320, skips=[4], L=10, Lv=4), dict(D=12, W=96, skips=[3, 6, 9], L=5, Lv=2),
          dict(D=8, W=256, skips=[4], L=12, Lv=6), dict(D=9, W=272, skips=[4], L=10, Lv=0)]
R, S = 21, 37                                        # 777 rows


def build(P, shape, precision, seed=47):
    D, Wd, skips, Lx, Lv = shape["D"], shape["W"], shape["skips"], shape["L"], shape["Lv"]
    torch.manual_seed(seed)
    emb_fn, in_ch = P.get_embedder(Lx, 0)
    embd_fn, in_ch_v = P.get_embedder(Lv, 0) if Lv > 0 else (None, 0)
    net = P.NeRF(D=D, W=Wd, input_ch=in_ch, input_ch_views=in_ch_v, output_ch=5, skips=skips, use_viewdirs=Lv > 0,
                 precision=precision).to(dev())
    assert not net.is_supported()
    return net, emb_fn, embd_fn


def inputs():
    gen = torch.Generator().manual_seed(53)
    pts = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    cot = torch.randn(R, S, 4, generator=gen)
    return pts, vd, cot


_REFERENCES = {}


class ReluTaking(torch.autograd.Function):
    """relu(z) whose backward takes the branch `branch` says (a bool per element) instead of z > 0."""

    @staticmethod
    def forward(ctx, z, branch):
        ctx.save_for_backward(branch)
        return torch.relu(z)

    @staticmethod
    def backward(ctx, grad):
        return grad * ctx.saved_tensors[0].to(grad.dtype), None


def reference(P, k):
    """Shape k in fp64 torch, once: (state dict, forward(params, branches) -> (output, the ReLU layers' pre-activations in
    the route's order: the trunk's, then the view layer's), output)."""
    if k in _REFERENCES:
        return _REFERENCES[k]
    F = torch.nn.functional
    shape = SHAPES[k]
    net, emb_fn, embd_fn = build(P, shape, "f16x3")
    sd = {n: v.detach().cpu().double() for n, v in net.state_dict().items()}
    pts, vd, _ = inputs()
    x = emb_fn(pts.reshape(-1, 3).double())
    v = embd_fn(vd[:, None].expand(R, S, 3).reshape(-1, 3).double()) if shape["Lv"] > 0 else None

    def forward(params, branches=None):
        pre, h = [], x

        def relu(z):
            pre.append(z)
            return F.relu(z) if branches is None else ReluTaking.apply(z, branches[len(pre) - 1])
        for i in range(shape["D"]):
            h = relu(F.linear(h, params[f"pts_linears.{i}.weight"], params[f"pts_linears.{i}.bias"]))
            if i in shape["skips"]:
                h = torch.cat([x, h], -1)
        if v is None:
            return F.linear(h, params["output_linear.weight"], params["output_linear.bias"]), pre
        sigma = F.linear(h, params["alpha_linear.weight"], params["alpha_linear.bias"])
        feat = F.linear(h, params["feature_linear.weight"], params["feature_linear.bias"])
        hv = relu(F.linear(torch.cat([feat, v], -1), params["views_linears.0.weight"], params["views_linears.0.bias"]))
        return torch.cat([F.linear(hv, params["rgb_linear.weight"], params["rgb_linear.bias"]), sigma], -1), pre
    with torch.no_grad():
        out, pre = forward(sd)
    _REFERENCES[k] = (sd, forward, out, [z.detach() for z in pre])
    return _REFERENCES[k]
