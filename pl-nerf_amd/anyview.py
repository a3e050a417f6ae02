"""The host side of plnerf_render_view_any (include/experimental/plnerf_hip_anyview.h): one library call per rendered frame
for ANY pair of networks create_nerf builds -- each of the two on the compiled 8 x 256 trunk or outside it (netwidth > 256,
netdepth > 8, several live skips, more than 10 | 4 frequency bands) -- where view.ViewRenderer serves the pair on the trunk
only.  The commonest such pair is a mixed one: --netwidth 256 --netwidth_fine 512.

`AnyViewRenderer` is view.ViewRenderer with a route per network slot, on the same base (onecall.Renderer owns the frame
planes, the workspace, the linspace tables and the structs).  A slot's route is the one NeRF.forward would take under the
switches of generic.py AS THEY ARE WHEN THE RENDERER IS BUILT:

    the compiled trunk (is_native)                          FUSED      plnerf_mlp_fwd in the network's precision
    outside it, generic.honours(net)                        CHAIN16    plnerf_generic_fwd in the network's 16-bit precision
    outside it otherwise                                    LAYERS32   plnerf_generic_fwd_f32 (exact fp32, whatever `precision`)

(the bits of the layered 16-bit route and of generic.CHAIN_INFERENCE are the same, so that switch does not matter).  A frame
is what render() computes under functional.DrawSource(seed, 0, step) for the same pose given as a device tensor, bit for bit,
as view.py says of ViewRenderer; it depends neither on `chunk` nor on `max_net_rows`.  (Bit for bit where the fp32 reciprocal of
each focal length, 1.0f / float(f), which the entries' rays multiply by, is float(1.0 / f), which torch's device kernels
multiply by -- 11.3, 9.7, 1111.111 are such numbers; 10.77 is not, and there the two frames agree to rounding only.
evaluate.render_images_with_metrics(one_call=True), which promises render()'s rows, looks before it takes this route.)
"""
import ctypes

import torch

from . import _lib as L
from . import generic
from .nerf import Embedder
from .onecall import Renderer, fill_pinhole, fill_sampling, refusal_head
from .render import MAX_ROWS_PER_LAUNCH, _fusable
from .view import ViewRenderer

ROUTES = {L.ANYVIEW_FUSED: "fused", L.ANYVIEW_CHAIN16: "chain16", L.ANYVIEW_LAYERS32: "layers32"}
MAX_FREQS = 16      # plnerf_embed_rows' limit on either encoding


def _route(net, emb):
    """(route, None) of one network under the switches as they are, or (None, why it cannot be served)."""
    if net.is_native():
        if not (net.density_beta == 0.0 and _fusable(net, emb[0], emb[1], True)):
            return None, "a network on the fused trunk needs the in-kernel encoding, view directions and no density activation"
        if not all(p.is_cuda for p in net.param_list()):
            return None, "the networks must live on the GPU"
        return L.ANYVIEW_FUSED, None
    if net.is_supported():
        return None, "a network is padded into the fused trunk (neither the trunk itself nor outside it)"
    if not generic._describable(net):
        return None, "a network outside the fused trunk has more live skips than the one-call entries hold, or one behind its last layer"
    if not net.use_viewdirs or net.input_ch_cam != 0 or net.density_activation is not None:
        return None, "a network outside the fused trunk needs view directions, no camera code and no density activation"
    for e, width in ((emb[0], net.input_ch), (emb[1], net.input_ch_views)):
        if not (isinstance(e, Embedder) and e.is_standard(e.num_freqs) and 0 <= e.num_freqs <= MAX_FREQS and
                width == 3 + 6 * e.num_freqs):
            return None, f"a network outside the fused trunk needs the standard Embedder pair of at most {MAX_FREQS} bands"
    if not all(p.is_cuda for p in net.parameters()):
        return None, "the networks must live on the GPU"
    return (L.ANYVIEW_CHAIN16 if generic.honours(net) else L.ANYVIEW_LAYERS32), None


class AnyViewRenderer(Renderer):
    """Frames of H x W views through plnerf_render_view_any.  The arguments are ViewRenderer's; max_net_rows bounds the rows
    one call of a network outside the trunk takes (and with them the workspace: at 32,768 rays x 192 samples and W = 512
    the unbounded buffers would be tens of GB)."""
    ENTRY, IO, ARGS, FALLBACK = "plnerf_render_view_any", L.AnyViewIo, L.ViewArgs, "render()"

    @staticmethod
    def unsupported_reason(render_kwargs):
        """Why plnerf_render_view_any cannot serve this configuration (None: it can)."""
        kw = render_kwargs
        why = refusal_head(kw, 1024, constant=bool(kw.get("constant_init")))
        if why is not None:
            return why
        if kw.get("pytest", False) or kw.get("retraw", False) or kw.get("c2w_staticcam") is not None:
            return "pytest draws, retraw and c2w_staticcam stay with render()"
        emb = getattr(kw.get("network_query_fn"), "embedders", None)      # (create_nerf's query function says what it encodes with)
        if emb is None:
            return "network_query_fn does not name its encoders (create_nerf's does)"
        c, f = kw["network_fn"], kw["network_fine"]
        routes = []
        for n in (c, f):
            route, why = _route(n, emb)
            if why is not None:
                return why
            routes.append(route)
        if routes == [L.ANYVIEW_FUSED] * 2 and c.precision != f.precision:
            return "two networks on the fused trunk must run in one precision"
        if (c.input_ch, c.input_ch_views) != (f.input_ch, f.input_ch_views):
            return "both networks must read rows of the same widths"
        return None

    def __init__(self, render_kwargs, H, W, K, chunk, near, far, ndc=False, seed=0, max_net_rows=MAX_ROWS_PER_LAUNCH):
        kw = self._accepted(render_kwargs)
        emb = self._encoders = kw["network_query_fn"].embedders
        nets = (kw["network_fn"], kw["network_fine"])
        self.routes = tuple(_route(n, emb)[0] for n in nets)
        self.max_net_rows = int(max_net_rows)
        cfg = L.StepConfig()
        constant = kw["mode"] == "constant" or bool(kw.get("constant_init", False))      # (run_plnerf.py:710-711)
        fused = [n for n, r in zip(nets, self.routes) if r == L.ANYVIEW_FUSED]
        # (the config's precision and widths are the fused slots'; without one the entry ignores them)
        fill_sampling(cfg, kw, chunk, fused[0] if fused else nets[0], seed, mode="constant" if constant else "linear")
        if not fused:
            cfg.precision = L.PRECISION["fp32"]
        fill_pinhole(cfg, ndc, K, H, W, near, far)
        self._build(kw, cfg, H, W, far)

    # ---- what differs from two networks of the trunk: how a slot is bound, sized, checked for having moved, and read
    def _bind_networks(self):
        cfg, io, dev = self.config, self.io, self.device
        io.max_net_rows = self.max_net_rows
        self._precisions = tuple(n.precision for n in self.nets)
        self._status_off = L.lib().plnerf_mlp_status_offset(cfg.precision) // 4
        packed, params, tables = [], [], []
        for slot, net, route in zip((io.coarse, io.fine), self.nets, self.routes):
            slot.route = route
            if route == L.ANYVIEW_FUSED:
                # (the renderer's own packed buffer, zeroed once: the kernels only ever OR into the status word)
                buf = torch.zeros(L.lib().plnerf_mlp_packed_bytes(cfg.precision) // 4, device=dev, dtype=torch.float32)
                live = [p.detach() for p in net.param_list()]
                for k, p in enumerate(live):
                    slot.fused.params[k] = L.dptr(p, f"params[{k}]").value
                slot.fused.packed = buf.data_ptr()
                packed.append(buf), params.append(live), tables.append(None)
                continue
            live = [t for fc in generic._layers(net) for t in (fc.weight, fc.bias)]
            fp32, table = generic._param_table(live)
            shape = generic._describe(net, torch.empty(0, net.input_ch + net.view_ch, device=dev))[0]
            ctypes.memmove(ctypes.byref(slot.shape), ctypes.byref(shape), ctypes.sizeof(shape))
            slot.params = ctypes.cast(table, ctypes.c_void_p).value
            if route == L.ANYVIEW_CHAIN16:
                slot.precision = L.PRECISION[net.precision]
                slot.status = net.status_word().data_ptr()
            packed.append(None), params.append([p.detach() for p in live]), tables.append((fp32, table))
        # (_tables: the fp32 tensors and the host table the slot points at, alive as long as the renderer)
        self.packed, self._params, self._tables = tuple(packed), tuple(params), tuple(tables)

    def _workspace_bytes(self):
        return L.lib().plnerf_render_view_any_workspace_bytes(ctypes.byref(self.config), ctypes.byref(self.io))

    def _live(self, net, route):
        if route == L.ANYVIEW_FUSED:
            return net.param_list()
        return [t for fc in generic._layers(net) for t in (fc.weight, fc.bias)]

    def current(self):
        """Do the structs still describe the live networks: their parameter addresses, their precisions, and the route each
        would take under the switches as they are NOW?"""
        for net, route, precision, params, tables in zip(self.nets, self.routes, self._precisions, self._params, self._tables):
            if _route(net, self._encoders)[0] != route or net.precision != precision:
                return False
            live = self._live(net, route)
            if len(live) != len(params) or any(p.data_ptr() != q.data_ptr() for p, q in zip(live, params)):
                return False
            # (a parameter that is not contiguous fp32 was copied into the table: the copy does not follow the network)
            if tables is not None and any(p.data_ptr() != t.data_ptr() for p, t in zip(live, tables[0])):
                return False
        return True

    def status_words(self):
        """(coarse, fine): a fused slot's word of the renderer's own packed buffer, a CHAIN16 slot's net.status_word(), None
        for a LAYERS32 slot (exact fp32 cannot leave a range)."""
        words = []
        for net, route, packed in zip(self.nets, self.routes, self.packed):
            if route == L.ANYVIEW_FUSED:
                words.append(packed.view(torch.int32)[self._status_off:self._status_off + 1])
            else:
                words.append(net.status_word() if route == L.ANYVIEW_CHAIN16 else None)
        return tuple(words)

    def check_range(self, bits=None):
        """ViewRenderer.check_range per network: a clamped frame must not pass silently.  bits: the two words as host
        integers (0 for a slot without one); None reads them from the device (synchronises)."""
        words = self.status_words()
        if bits is None:
            bits = [0 if (word is None or net.precision not in L.GUARDED_PRECISIONS) else int(word.item())
                    for word, net in zip(words, self.nets)]
        for b, word, which, net, route in zip(bits, words, ("coarse", "fine"), self.nets, self.routes):
            if b and word is not None:
                word.zero_()
                raise FloatingPointError(
                    f"plnerf_amd: the {which} network ({ROUTES[route]}) left the IEEE-half range while rendering (status {b}, "
                    f"precision={net.precision!r}): the frame was clamped.  Use precision='bf16x3' or 'fp32' for this network.")

    # a frame is enqueued, checked and returned as ViewRenderer's: the entry differs, not the call
    enqueue, render = ViewRenderer.enqueue, ViewRenderer.render


def frame_renderer(render_kwargs, H, W, K, chunk, near, far, ndc=False, seed=0, max_net_rows=MAX_ROWS_PER_LAUNCH):
    """The one-call renderer that serves this configuration: view.ViewRenderer where it can (unchanged), else AnyViewRenderer,
    else None (render() remains)."""
    if ViewRenderer.supported(render_kwargs):
        return ViewRenderer(render_kwargs, H, W, K, chunk, near, far, ndc=ndc, seed=seed)
    if AnyViewRenderer.supported(render_kwargs):
        return AnyViewRenderer(render_kwargs, H, W, K, chunk, near, far, ndc=ndc, seed=seed, max_net_rows=max_net_rows)
    return None
