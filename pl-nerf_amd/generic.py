"""NeRF shapes outside the compiled trunk, layer by layer on the HIP path.

The reference's `NeRF` (run_nerf_helpers.py:76-128) builds any netdepth / netwidth / skip list / encoding width
(flags run_plnerf.py:784-825).  The fused kernels serve the trunk every shipped configuration uses and what maps onto it
exactly (nerf.NeRF.param_list); a network that does not -- netwidth > 256, netdepth > 8, several live skips, multires > 10,
multires_views > 4 -- runs here: every nn.Linear as ONE exact-fp32 MFMA product (plnerf_gemm_f32: bias and ReLU in its
epilogue), its backward as two more (the ReLU's derivative gated into their first operand, the bias gradient as an extra
column of the weight gradient), the concatenations as torch.cat (autograd splits their gradients), the positional encoding
as plnerf_embed_rows.  Unfused -- every layer's activations make a round trip through HBM -- and fp32 whatever `precision`
says: a correct native route for shapes no shipped configuration uses, several times slower per row than the fused
kernels.  No CPU fallback here either."""
import torch

from . import _lib as L

# Opt-in: a generic network whose `precision` is one of the 16-bit modes runs its FORWARD products in that arithmetic
# (plnerf_gemm_h16: operands split on the fly, hi.hi + lo.hi + hi.lo per k-step; the plain modes the one rounded product) and
# owns a range status word (nerf.NeRF.status_word).  The backward stays on plnerf_gemm_f32 over the fp32 activations the
# forward wrote.  Off (the default): every product is plnerf_gemm_f32 whatever `precision` says, bit for bit as before.
# Set it BEFORE create_nerf: that is where the optimizers are handed the networks that guard their steps (render.create_nerf's
# guard()), and a network outside the trunk is among them only if the switch is on then.  Switched on later, a clamped
# forward still sets the word and check_range() still raises, but the Adam step is not withheld.
# (A module switch like render.FUSE_CONST_EPILOGUE; tests set and restore it.)
HONOUR_PRECISION = False

# Opt-in, on top of HONOUR_PRECISION: where a layer's forward ran on plnerf_gemm_h16 (HONOUR_PRECISION on, a 16-bit
# `precision`), its two BACKWARD products run in the same arithmetic (plnerf_gemm_h16_dgrad / _wgrad: the gated gradient and
# the other operand split on the fly, hi.hi + lo.hi + hi.lo per 16-deep step in the x3 modes) and OR into the same status
# word, so the guarded Adam withholds a step a backward product clamped like one a forward did.  In the IEEE-half modes the
# gradient is scaled into the half range by a power of two taken from max |g| (one device scalar per layer and backward
# call, no host sync).  Off (the default), or without HONOUR_PRECISION, or in an fp32 network: no effect -- the backward is
# plnerf_gemm_f32, bit for bit as before.  Read when a layer's forward runs, so it may be switched between steps.
HONOUR_PRECISION_BACKWARD = False
_HALF = ("f16x3", "f16")      # IEEE-half elements: the backward entries are handed max |g|

# Opt-in, on top of HONOUR_PRECISION: a forward that autograd would not record (grad mode off, or neither the rows nor a
# parameter requires grad) is ONE plnerf_generic_fwd call per chunk instead of one plnerf_gemm_h16 per layer: the weights are
# split once per call, the activations stay 16-bit planes in a workspace cached on the network, no torch op sits between the
# layers.  The results are the layered route's bit for bit (the same clamp and split, applied by the producing layer's
# epilogue instead of the consuming layer's loader) and the same bits of the status word are raised.  Off (the default), or
# without HONOUR_PRECISION, or in an fp32 network, or whenever autograd records: no effect.  Read at every forward.
CHAIN_INFERENCE = False

# Opt-in, on top of HONOUR_PRECISION and HONOUR_PRECISION_BACKWARD: a TRAINING forward (grad mode on, a parameter that
# requires grad, rows that do not) is ONE plnerf_generic_train_fwd call and its backward ONE plnerf_generic_train_bwd call,
# wrapped in one autograd.Function for the whole network: the forward keeps every layer's output as the 16-bit planes it
# produces (plus one gate bit per element) in a state allocated per call, and the backward reads those planes instead of
# splitting fp32 activations again.  Outputs, gradients and status bits are the layered 16-bit route's bit for bit.  Off (the
# default), or without either of the two switches above, or in an fp32 network, or with rows that require grad (pose or input
# gradients): no effect -- the layered route runs.  Read at every forward.
CHAIN_TRAINING = False


def honours(net):
    """True when `net`'s forward through this route runs in its own 16-bit precision (and has a range status word)."""
    return HONOUR_PRECISION and net.precision in L.GUARDED_PRECISIONS


def _splits(M, N, K):
    tiles = -(-M // 64) * -(-N // 64)
    return max(1, min(1024 // tiles, K // 512)) if tiles < 256 else 1


def _gemm(a, a_rs, a_cs, b, b_rs, b_cs, M, N, K, bias=None, gate=None, relu=False, ones_col=False, out=None):
    c = torch.empty(M, N, device=a.device, dtype=torch.float32) if out is None else out
    if M == 0 or N == 0:
        return c
    # a product with few 64 x 64 output tiles and a long k (a weight gradient: k = the rows): deal k out so that ~1000
    # workgroups share it (64 of them walking 262,144 rows each measured 430 ms per backward at 8 x 512)
    splits = _splits(M, N, K)
    partials = torch.empty(splits * M * N, device=a.device, dtype=torch.float32) if splits > 1 else None
    L.check(L.lib().plnerf_gemm_f32(L.dptr(a, "a"), a_rs, a_cs, L.dptr(b, "b"), b_rs, b_cs, L.dptr(bias, "bias"), L.dptr(gate, "gate"),
                                    M, N, K, int(relu), 0, int(ones_col), L.dptr(c, "c"), c.stride(0), splits,
                                    L.dptr(partials, "partials"), L.stream()), "plnerf_gemm_f32")
    return c


def _rows(t, name):
    """Device pointer and row stride of a 2-D fp32 tensor whose rows are contiguous (a column slice of wider rows included:
    plnerf_gemm_h16 takes the row stride, so no copy is made)."""
    if not t.is_cuda:
        raise RuntimeError(f"plnerf_amd: `{name}` is on {t.device}; the HIP path needs a GPU tensor (there is no CPU fallback)")
    return L.ctypes.c_void_p(t.data_ptr()), t.stride(0)


def _gemm_h16(x, w, bias, relu, precision, status):
    """relu?(x W^T + bias) in a 16-bit mode's arithmetic (plnerf_gemm_h16); x and w may be column slices of wider rows."""
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    if M == 0 or N == 0:
        return y
    if M > 1 and x.stride(0) < K or N > 1 and w.stride(0) < K:      # (an expanded view: rows that overlap)
        raise RuntimeError("plnerf_amd: plnerf_gemm_h16 needs rows at least K apart")
    (a_ptr, lda), (w_ptr, ldw) = _rows(x, "x"), _rows(w, "weight")
    L.check(L.lib().plnerf_gemm_h16(a_ptr, max(lda, K), w_ptr, max(ldw, K), L.dptr(bias, "bias"), M, N, K, int(relu),
                                    L.PRECISION[precision], L.dptr(y, "y"), y.stride(0), L.dptr(status, "status", torch.int32),
                                    L.stream()), "plnerf_gemm_h16")
    return y


def _rows_h16(t, width, name):
    """`t` as the 16-bit entries read it: fp32, rows contiguous and at least `width` apart (a column slice stays in place)."""
    t = t.to(torch.float32)
    if not (t.dim() == 2 and t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= width)):
        t = t.contiguous()
    ptr, ld = _rows(t, name)
    return t, ptr, max(ld, width)


def _backward_h16(g, y, x, w, precision, status, need_x, need_w):
    """(dx, [dW | db]) of one layer in a 16-bit mode's arithmetic: plnerf_gemm_h16_dgrad / _wgrad.  The ReLU gate (y, or
    None) is applied in the kernels' loaders; max |g| -- IEEE-half modes only -- is one device scalar shared by both."""
    M, K = x.shape
    N = w.shape[0]
    g, g_ptr, ldg = _rows_h16(g, N, "grad")
    (y_ptr, ldy) = _rows(y, "y") if y is not None else (None, 0)
    absmax = torch.linalg.vector_norm(g, ord=float("inf")) if precision in _HALF and g.numel() else None
    code, word, gx, gwb = L.PRECISION[precision], L.dptr(status, "status", torch.int32), None, None
    if need_x:
        gx = torch.empty(M, K, device=g.device, dtype=torch.float32)
        w_ptr, ldw = _rows(w, "weight")
        L.check(L.lib().plnerf_gemm_h16_dgrad(g_ptr, ldg, y_ptr, ldy, w_ptr, max(ldw, K), M, N, K, code, L.dptr(absmax, "absmax"),
                                              L.dptr(gx, "gx"), max(K, 1), word, L.stream()), "plnerf_gemm_h16_dgrad")
    if need_w:
        gwb = torch.empty(N, K + 1, device=g.device, dtype=torch.float32)
        splits = _splits(N, K + 1, M)
        partials = torch.empty(splits * N * (K + 1), device=g.device, dtype=torch.float32) if splits > 1 else None
        x_ptr, ldx = _rows(x, "x")
        L.check(L.lib().plnerf_gemm_h16_wgrad(g_ptr, ldg, y_ptr, ldy, x_ptr, max(ldx, K), M, N, K, code, L.dptr(absmax, "absmax"),
                                              L.dptr(gwb, "gwb"), K + 1, splits, L.dptr(partials, "partials"), word,
                                              L.stream()), "plnerf_gemm_h16_wgrad")
    return gx, gwb


class LinearFn(torch.autograd.Function):
    """y = relu?(x W^T + b) as one plnerf_gemm_f32 (with HONOUR_PRECISION and a 16-bit `precision`: one plnerf_gemm_h16, which
    ORs into `status`); backward: dx = (g * [y > 0]) W, [dW | db] = (g * [y > 0])^T [x | 1], on plnerf_gemm_f32 -- or, where
    the forward ran on plnerf_gemm_h16 and HONOUR_PRECISION_BACKWARD is on, on plnerf_gemm_h16_dgrad / _wgrad."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, precision="fp32", status=None):
        h16 = HONOUR_PRECISION and precision != "fp32"
        x = x.detach().to(torch.float32)
        w = weight.detach().to(torch.float32)
        if not (h16 and x.dim() == 2 and x.stride(1) == 1):      # (the 16-bit entry reads a column slice in place)
            x = x.contiguous()
        if not (h16 and w.dim() == 2 and w.stride(1) == 1):
            w = w.contiguous()
        M, K = x.shape
        N = w.shape[0]
        if w.shape[1] != K:      # (as F.linear: e.g. a skip after the LAST trunk layer, whose concatenation no head layer takes)
            raise RuntimeError(f"plnerf_amd: a layer with {w.shape[1]} input features got rows of {K}")
        b = bias.detach().to(torch.float32).contiguous()
        ctx.h16_backward = bool(h16 and HONOUR_PRECISION_BACKWARD)
        ctx.precision, ctx.status = precision, status
        if h16:
            y = _gemm_h16(x, w, b, relu, precision, status)
            if not ctx.h16_backward:      # (the 16-bit backward entries take row strides: a column slice is read in place)
                x, w = x.contiguous(), w.contiguous()      # (what the fp32 products index; a no-op but for a column slice)
        else:
            # B(k, j) = W[j, k]: row stride 1, column stride K
            y = _gemm(x, K, 1, w, 1, K, M, N, K, bias=b, relu=relu)
        ctx.relu = bool(relu)
        ctx.save_for_backward(x, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, y = ctx.saved_tensors
        M, K = x.shape
        N = w.shape[0]
        if ctx.h16_backward:
            gx, gwb = _backward_h16(g, y, x, w, ctx.precision, ctx.status, ctx.needs_input_grad[0],
                                    ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
            gw = gwb[:, :K].contiguous() if gwb is not None and ctx.needs_input_grad[1] else None
            gb = gwb[:, K].contiguous() if gwb is not None and ctx.needs_input_grad[2] else None
            return gx, gw, gb, None, None, None
        g = g.to(torch.float32).contiguous()
        gx = gwb = None
        if ctx.needs_input_grad[0]:
            # dx[M, K] = gate(g)[M, N] . W[N, K]
            gx = _gemm(g, N, 1, w, K, 1, M, K, N, gate=y)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            # [dW | db][N, K + 1] = gate(g)^T[N, M] . [x | 1][M, K + 1]: A(i = n, k = m) = g[m, n]
            gwb = _gemm(g, 1, N, x, K, 1, N, K + 1, M, gate=y, ones_col=True)
        gw = gwb[:, :K].contiguous() if gwb is not None and ctx.needs_input_grad[1] else None
        gb = gwb[:, K].contiguous() if gwb is not None and ctx.needs_input_grad[2] else None
        return gx, gw, gb, None, None, None


def linear(x, layer, relu, precision="fp32", status=None):
    if not x.is_cuda:
        raise RuntimeError(f"plnerf_amd: the generic NeRF route got a tensor on {x.device}; the HIP path needs a GPU tensor "
                           "(there is no CPU fallback)")
    return LinearFn.apply(x, layer.weight, layer.bias, relu, precision, status)


def _softplus_density(cols, at):
    """F.softplus(beta=10) on column `at` (the depth-supervised variant's density channel, model/run_nerf_helpers.py:200)."""
    return torch.cat([cols[:, :at], torch.nn.functional.softplus(cols[:, at:at + 1], beta=10), cols[:, at + 1:]], 1)


def chains(net, rows):
    """True when forward(net, rows) takes the one-call entry: CHAIN_INFERENCE on a network that honours its precision, nothing
    for autograd to record, and a shape the entry describes (its skip list holds PLNERF_GENERIC_MAX_SKIPS entries; a skip
    behind the last trunk layer is left to the layered route, which names the layer that cannot consume it)."""
    if not (CHAIN_INFERENCE and honours(net)):
        return False
    if torch.is_grad_enabled() and (rows.requires_grad or any(p.requires_grad for p in net.parameters())):
        return False
    return _describable(net)


def chains_training(net, rows):
    """True when forward(net, rows) takes the one-call training entries: CHAIN_TRAINING on a network that honours its precision
    in both directions, a forward that autograd records for the parameters alone, and a shape chains() accepts."""
    if not (CHAIN_TRAINING and HONOUR_PRECISION_BACKWARD and honours(net)):
        return False
    if not torch.is_grad_enabled() or rows.requires_grad or not any(p.requires_grad for p in net.parameters()):
        return False
    return _describable(net)


def _live_skips(net):
    return sorted(set(k for k in net.skips if 0 <= k < net.D))


def _describable(net):
    """A shape plnerf_generic_shape holds and the one-call entries accept."""
    live = _live_skips(net)
    return len(live) <= L.GENERIC_MAX_SKIPS and net.D - 1 not in live


def _layers(net):
    """The modules in the order of the C entries' `params` and `grads` (the class's state_dict order)."""
    layers = list(net.pts_linears) + list(net.views_linears)
    return layers + ([net.feature_linear, net.alpha_linear, net.rgb_linear] if net.use_viewdirs else [net.output_linear])


def _describe(net, rows):
    """What the one-call entries are handed: (plnerf_generic_shape, rows as they read them, their pointer and row stride)."""
    if not rows.is_cuda:
        raise RuntimeError(f"plnerf_amd: the generic NeRF route got a tensor on {rows.device}; the HIP path needs a GPU tensor "
                           "(there is no CPU fallback)")
    rows, rows_ptr, ld_rows = _rows_h16(rows.detach(), net.input_ch + net.view_ch, "rows")
    live = _live_skips(net)
    shape = L.GenericShape(D=net.D, W=net.W, input_ch=net.input_ch, view_ch=net.view_ch, use_viewdirs=int(bool(net.use_viewdirs)),
                           output_ch=0 if net.use_viewdirs else net.output_linear.out_features,
                           n_view_layers=len(net.views_linears), n_skips=len(live))
    for q, k in enumerate(live):
        shape.skips[q] = k
    return shape, rows, rows_ptr, ld_rows


def _param_table(tensors):
    tensors = [t.detach().to(torch.float32).contiguous() for t in tensors]
    return tensors, (L.ctypes.c_void_p * len(tensors))(*[L.dptr(t, "parameter").value for t in tensors])


def _chain_forward(net, rows):
    """One plnerf_generic_fwd call: raw outputs [N, 4 or output_ch]."""
    shape, rows, rows_ptr, ld_rows = _describe(net, rows)
    n = rows.shape[0]
    tensors, params = _param_table([t for fc in _layers(net) for t in (fc.weight, fc.bias)])
    out = torch.empty(n, 4 if net.use_viewdirs else shape.output_ch, device=rows.device, dtype=torch.float32)
    if n == 0:
        return out
    code = L.PRECISION[net.precision]
    nbytes = L.lib().plnerf_generic_fwd_workspace_bytes(L.ctypes.byref(shape), n, code)
    if nbytes == 0:
        raise RuntimeError("plnerf_amd: plnerf_generic_fwd_workspace_bytes refused this network")
    ws = net.__dict__.get("_chain_workspace")      # (cached on the network and re-grown on demand, as _packed is)
    if ws is None or ws.device != rows.device or ws.numel() < nbytes:
        ws = net.__dict__["_chain_workspace"] = torch.empty(nbytes, device=rows.device, dtype=torch.uint8)
    L.check(L.lib().plnerf_generic_fwd(L.ctypes.byref(shape), params, rows_ptr, ld_rows, n, code, L.ctypes.c_void_p(ws.data_ptr()),
                                       ws.numel(), L.dptr(out, "out"), out.stride(0),
                                       L.dptr(net.status_word(), "status", torch.int32), L.stream()), "plnerf_generic_fwd")
    return out


class ChainTrainFn(torch.autograd.Function):
    """The whole network as one node: forward = one plnerf_generic_train_fwd call whose saved state (16-bit planes, gate bits,
    packed weights) is allocated per call and kept on ctx -- run_network calls a network once per netchunk before any backward
    runs --; backward = one plnerf_generic_train_bwd call into one [N, K + 1] block per layer.  apply(net, shape, rows,
    rows_ptr, ld_rows, *weights_and_biases)."""

    @staticmethod
    def forward(ctx, net, shape, rows, rows_ptr, ld_rows, *tensors):
        n = rows.shape[0]
        fp32, params = _param_table(tensors)      # (fp32: the tensors the table points at, alive across the call)
        code = L.PRECISION[net.precision]
        need = L.lib().plnerf_generic_train_saved_bytes(L.ctypes.byref(shape), n, code)
        if need == 0 and n > 0:
            raise RuntimeError("plnerf_amd: plnerf_generic_train_saved_bytes refused this network")
        saved = torch.empty(max(need, 16), device=rows.device, dtype=torch.uint8)
        out = torch.empty(n, 4 if shape.use_viewdirs else shape.output_ch, device=rows.device, dtype=torch.float32)
        status = net.status_word()
        L.check(L.lib().plnerf_generic_train_fwd(L.ctypes.byref(shape), params, rows_ptr, ld_rows, n, code,
                                                 L.ctypes.c_void_p(saved.data_ptr()), saved.numel(), L.dptr(out, "out"),
                                                 max(out.stride(0), out.shape[1]), L.dptr(status, "status", torch.int32),
                                                 L.stream()), "plnerf_generic_train_fwd")
        ctx.shape, ctx.rows, ctx.rows_ptr, ctx.ld_rows, ctx.code, ctx.saved, ctx.status = shape, rows, rows_ptr, ld_rows, code, saved, status
        ctx.dims = [tuple(t.shape) for t in tensors[0::2]]      # (N, K) per layer
        ctx.runs = [bool(shape.use_viewdirs) or not (shape.D <= q < shape.D + shape.n_view_layers) for q in range(len(ctx.dims))]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        shape, rows, code = ctx.shape, ctx.rows, ctx.code
        n = rows.shape[0]
        g, g_ptr, ld_g = _rows_h16(g, g.shape[1], "grad")
        need = L.lib().plnerf_generic_train_workspace_bytes(L.ctypes.byref(shape), n, code)
        ws = torch.empty(max(need, 16), device=g.device, dtype=torch.uint8)
        blocks = [torch.empty(N, K + 1, device=g.device, dtype=torch.float32) if run else None
                  for (N, K), run in zip(ctx.dims, ctx.runs)]
        grads = (L.ctypes.c_void_p * len(blocks))(*[None if b is None else b.data_ptr() for b in blocks])
        L.check(L.lib().plnerf_generic_train_bwd(L.ctypes.byref(shape), ctx.rows_ptr, ctx.ld_rows, n, code,
                                                 L.ctypes.c_void_p(ctx.saved.data_ptr()), ctx.saved.numel(), g_ptr, ld_g, grads,
                                                 L.ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                                 L.dptr(ctx.status, "status", torch.int32), L.stream()), "plnerf_generic_train_bwd")
        out = []
        for q, ((N, K), block) in enumerate(zip(ctx.dims, blocks)):
            need_w, need_b = ctx.needs_input_grad[5 + 2 * q], ctx.needs_input_grad[6 + 2 * q]
            out.append(block[:, :K].contiguous() if block is not None and need_w else None)
            out.append(block[:, K].contiguous() if block is not None and need_b else None)
        return (None, None, None, None, None, *out)


def _chain_train_forward(net, rows):
    """One plnerf_generic_train_fwd call under autograd: raw outputs [N, 4 or output_ch]."""
    shape, rows, rows_ptr, ld_rows = _describe(net, rows)
    return ChainTrainFn.apply(net, shape, rows, rows_ptr, ld_rows, *[t for fc in _layers(net) for t in (fc.weight, fc.bias)])


def forward(net, rows):
    """The module's layers applied to embedded rows [N, input_ch + view_ch], whatever its shape: what NeRF.forward computes
    (run_nerf_helpers.py:105-128; with the camera columns and the softplus density of the depth-supervised variant,
    depth_supervised_exps/model/run_nerf_helpers.py:164-205), every nn.Linear through LinearFn -- or, with CHAIN_INFERENCE and
    nothing for autograd to record, all of them in one plnerf_generic_fwd call -- or, with CHAIN_TRAINING and only the
    parameters to record for, in one plnerf_generic_train_fwd call whose backward is one plnerf_generic_train_bwd call."""
    if chains(net, rows) or chains_training(net, rows):
        out = _chain_forward(net, rows) if chains(net, rows) else _chain_train_forward(net, rows)
        return _softplus_density(out, 3) if net.density_activation == "softplus" else out
    # (with HONOUR_PRECISION: the network's 16-bit mode and its range status word, through every layer)
    mode = net.precision if honours(net) else "fp32"
    word = net.status_word() if mode != "fp32" else None

    def layer(x, fc, relu):
        return linear(x, fc, relu, mode, word)
    xyz = rows[:, :net.input_ch]
    act = xyz
    for depth, fc in enumerate(net.pts_linears):
        act = layer(act, fc, relu=True)
        if depth in net.skips:      # the encoding re-enters BEHIND this layer, its channels first (:111-112)
            act = torch.cat((xyz, act), 1)
    if not net.use_viewdirs:
        out = layer(act, net.output_linear, relu=False)
        return _softplus_density(out, 3) if net.density_activation == "softplus" else out
    sigma = layer(act, net.alpha_linear, relu=False)
    side = rows[:, net.input_ch:net.input_ch + net.view_ch]      # direction encoding (+ camera code)
    head = torch.cat((layer(act, net.feature_linear, relu=False), side), 1)
    for fc in net.views_linears:
        head = layer(head, fc, relu=True)
    out = torch.cat((layer(head, net.rgb_linear, relu=False), sigma), 1)
    return _softplus_density(out, 3) if net.density_activation == "softplus" else out
