"""The host side of plnerf_render_view (include/plnerf_hip_view.h): one library call per rendered frame, and frames that
leave the device as 8-bit colour / 16-bit depth.

`ViewRenderer` owns what the call needs beyond the two networks -- the frame planes, the workspace the library carves up,
both packed weight buffers, the two linspace tables -- and the three structs of the ABI, filled once.  A frame is one
call: it packs both networks' weights, walks the view in blocks of `chunk` pixels and quantises the result on the
device.  What it computes is what render() computes under functional.DrawSource(seed, 0, step) for the same pose GIVEN AS A
DEVICE TENSOR, bit for bit: render() builds its rays with rays.get_rays where the pose lives, and the call's rays are the
device's evaluation of that expression.  (For a host pose render() takes the host's get_rays, whose directions differ from
the device's by an ulp; the frames then agree to rounding, not bit for bit.)  Configurations outside the call (supported())
stay with render().

`render_path_frames` is render_path (run_plnerf.py:178-216) on that route, writing '{:03d}.png' per frame when asked to.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from . import functional as Fn
from .nerf import NeRF
from .png import write_png
from .render import _fusable


def _aligned(nbytes, device):
    """An fp32 tensor of at least `nbytes` bytes whose address is a multiple of the workspace alignment."""
    raw = torch.empty((nbytes + L.STEP_WORKSPACE_ALIGN) // 4 + 1, device=device, dtype=torch.float32)
    pad = (-raw.data_ptr()) % L.STEP_WORKSPACE_ALIGN
    return raw[pad // 4:]


class ViewRenderer:
    """Frames of H x W views through plnerf_render_view.  render_kwargs: create_nerf's dict (render_kwargs_test, say);
    K: the 3 x 3 intrinsics; chunk: pixels per block (render()'s chunk); near / far / ndc as render() takes them.  A frame
    is render()'s for a device-resident c2w under DrawSource(seed, 0, step), bit for bit (the module docstring has the
    condition); the pose handed to render() / enqueue() here may live anywhere, 12 host floats are read from it."""

    @staticmethod
    def unsupported_reason(render_kwargs):
        """Why plnerf_render_view cannot serve this configuration (None: it can)."""
        kw = render_kwargs
        c, f = kw.get("network_fn"), kw.get("network_fine")
        if not (isinstance(c, NeRF) and isinstance(f, NeRF)) or c is f:
            return "two networks (network_fn and network_fine) of the package's NeRF class are needed"
        if int(kw.get("N_importance", 0)) < 1:
            return "N_importance must be at least 1"
        if not kw.get("use_viewdirs", False):
            return "use_viewdirs must be set"
        if kw.get("mode") not in ("linear", "constant") or kw.get("color_mode", "midpoint") not in ("midpoint", "left"):
            return "mode must be linear or constant, color_mode midpoint or left"
        S, N = int(kw["N_samples"]), int(kw["N_importance"])
        if S < (3 if kw["mode"] == "constant" or kw.get("constant_init") else 2) or S + N > 1024:
            return "the sample counts are outside the kernels' limits"
        if kw.get("pytest", False) or kw.get("retraw", False) or kw.get("c2w_staticcam") is not None:
            return "pytest draws, retraw and c2w_staticcam stay with render()"
        emb = getattr(kw.get("network_query_fn"), "embedders", None)      # (create_nerf's query function says what it encodes with)
        if emb is None:
            return "network_query_fn does not name its encoders (create_nerf's does)"
        if c.precision != f.precision:
            return "both networks must run in one precision"
        for n in (c, f):
            if not (n.is_native() and n.density_beta == 0.0 and _fusable(n, emb[0], emb[1], True)):
                return "a network is outside the fused trunk with the in-kernel encoding and view directions"
            if not all(p.is_cuda for p in n.param_list()):
                return "the networks must live on the GPU"
        return None

    @staticmethod
    def supported(render_kwargs):
        return ViewRenderer.unsupported_reason(render_kwargs) is None

    def __init__(self, render_kwargs, H, W, K, chunk, near, far, ndc=False, seed=0):
        why = self.unsupported_reason(render_kwargs)
        if why is not None:
            raise ValueError(f"ViewRenderer: {why}; use render()")
        kw = render_kwargs
        self.nets = (kw["network_fn"], kw["network_fine"])
        coarse = self.nets[0]
        dev = coarse.param_list()[0].device
        self.device, self.H, self.W, self.far = dev, int(H), int(W), float(far)
        self.precision = coarse.precision
        cfg = self.config = L.StepConfig()
        cfg.max_rays, cfg.n_samples, cfg.n_importance = int(chunk), int(kw["N_samples"]), int(kw["N_importance"])
        constant = kw["mode"] == "constant" or bool(kw.get("constant_init", False))      # (run_plnerf.py:710-711)
        cfg.mode, cfg.color_mode = L.MODE["constant" if constant else "linear"], L.COLOR[kw.get("color_mode", "midpoint")]
        cfg.lindisp, cfg.perturb = int(bool(kw.get("lindisp", False))), int(kw.get("perturb", 0.) > 0.)
        cfg.white_bkgd, cfg.farcolorfix = int(bool(kw.get("white_bkgd", False))), int(bool(kw.get("farcolorfix", False)))
        cfg.raw_noise_std = float(kw.get("raw_noise_std", 0.))
        cfg.zero_tol, cfg.epsilon = float(kw.get("zero_tol", 1e-4)), float(kw.get("epsilon", 1e-3))
        cfg.ndc, cfg.ndc_focal = int(bool(ndc)), float(K[0][0])
        cfg.H, cfg.W = int(H), int(W)
        cfg.fx, cfg.fy, cfg.cx, cfg.cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
        cfg.near, cfg.far = float(near), float(far)
        cfg.precision, cfg.fwd_kernel = L.PRECISION[coarse.precision], L.FWD_KERNEL
        cfg.input_ch, cfg.input_ch_views = int(coarse.input_ch), int(coarse.hip_view_ch)
        cfg.seed = int(seed)
        nbytes = L.lib().plnerf_render_view_workspace_bytes(ctypes.byref(cfg))
        if nbytes == 0:
            raise ValueError("ViewRenderer: plnerf_render_view refuses this configuration; use render()")
        self.workspace, self.workspace_bytes = _aligned(nbytes, dev), nbytes
        self.t_vals = Fn.cpu_linspace(cfg.n_samples, dev)
        self.u_vals = Fn.cpu_linspace(cfg.n_importance, dev)
        n = self.H * self.W
        self.planes = {name: torch.empty((n, 3) if name in ("rgb", "rgb0") else (n,), device=dev) for name in L.VIEW_PLANES}
        self.rgb8 = torch.empty(n, 3, device=dev, dtype=torch.uint8)
        self.depth16 = torch.empty(n, device=dev, dtype=torch.int16)      # (uint16 bit patterns)
        # the renderer's own packed buffers (zeroed once: the kernels only ever OR into the status word)
        packed_bytes = L.lib().plnerf_mlp_packed_bytes(cfg.precision)
        self.packed = tuple(torch.zeros(packed_bytes // 4, device=dev, dtype=torch.float32) for _ in range(2))
        self._status_off = L.lib().plnerf_mlp_status_offset(cfg.precision) // 4
        io = self.io = L.ViewIo()
        self._params = tuple([p.detach() for p in net.param_list()] for net in self.nets)
        for io_net, params, packed in zip((io.coarse, io.fine), self._params, self.packed):
            for k, p in enumerate(params):
                io_net.params[k] = L.dptr(p, f"params[{k}]").value
            io_net.packed = packed.data_ptr()
        io.t_vals, io.u_vals = self.t_vals.data_ptr(), self.u_vals.data_ptr()
        for name in L.VIEW_PLANES:
            setattr(io, name, self.planes[name].data_ptr())
        self.args = L.ViewArgs()
        self.args.pack_weights = 1
        self.args.depth16_scale = float(np.float32(1.0) / np.float32(far))
        self._refs = (ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(self.args), ctypes.c_void_p(self.workspace.data_ptr()))

    def current(self):
        """Do the parameter addresses the structs hold still belong to the live networks (a .to() or a precision change
        moves them)?"""
        return all(net.precision == self.precision and
                   all(p.data_ptr() == q.data_ptr() for p, q in zip(net.param_list(), params))
                   for net, params in zip(self.nets, self._params))

    def status_words(self):
        """Both packed buffers' range status words, (coarse, fine), as 1-element int32 views."""
        return tuple(p.view(torch.int32)[self._status_off:self._status_off + 1] for p in self.packed)

    def check_range(self, bits=None):
        """render_path's check for the guarded precisions: a clamped frame must not pass silently.  bits: the two status
        words as host integers (a caller that copied them itself); None reads them from the device (synchronises)."""
        if self.precision not in L.GUARDED_PRECISIONS:
            return
        if bits is None:
            bits = [int(word.item()) for word in self.status_words()]
        for b, word, which in zip(bits, self.status_words(), ("coarse", "fine")):
            if b:
                word.zero_()
                raise FloatingPointError(
                    f"plnerf_amd: the {which} network left the IEEE-half range while rendering (status {b}, precision="
                    f"{self.precision!r}): the frame was clamped.  Use precision='bf16x3' or 'fp32' for this network.")

    def enqueue(self, c2w, step=0, export=False, pix0=0, n_pix=None):
        """Enqueue pixels [pix0, pix0 + n_pix) of the view `c2w` on the current stream (the whole view by default); nothing
        is synchronised.  The planes (self.planes, self.rgb8, self.depth16) hold the result once the stream gets there."""
        if not self.current():
            raise RuntimeError("ViewRenderer: the networks' parameters moved; build a new ViewRenderer")
        a = self.args
        a.c2w[:] = [float(v) for v in torch.as_tensor(c2w, device="cpu")[:3, :4].reshape(-1)]
        a.step, a.pix0 = int(step), int(pix0)
        a.n_pix = self.H * self.W - int(pix0) if n_pix is None else int(n_pix)
        self.io.rgb8 = self.rgb8.data_ptr() if export else None
        self.io.depth16 = self.depth16.data_ptr() if export else None
        cfg, io, args, ws = self._refs
        L.check(L.lib().plnerf_render_view(cfg, io, args, ws, self.workspace_bytes, L.stream()), "plnerf_render_view")

    def render(self, c2w, step=0, export=False):
        """[rgb_map, disp_map, acc_map, extras] of the full view, shaped like render()'s result; every tensor is a view
        of this renderer's planes (valid until its next frame).  extras: rgb0, disp0, acc0, depth0, depth_map, z_std,
        and with export=True rgb8 [H,W,3] uint8 and depth16 [H,W] (int16 holding the uint16 codes of depth / far)."""
        with torch.no_grad():
            self.enqueue(c2w, step, export)
            self.check_range()
        H, W, p = self.H, self.W, self.planes
        shaped = {k: (v.view(H, W, 3) if v.dim() == 2 else v.view(H, W)) for k, v in p.items()}
        extras = {"rgb0": shaped["rgb0"], "disp0": shaped["disp0"], "acc0": shaped["acc0"], "depth0": shaped["depth0"],
                  "depth_map": shaped["depth"], "z_std": shaped["z_std"]}
        if export:
            extras["rgb8"], extras["depth16"] = self.rgb8.view(H, W, 3), self.depth16.view(H, W)
        return [shaped["rgb"], shaped["disp"], shaped["acc"], extras]


def depth16_numpy(depth16):
    """ViewRenderer's depth16 plane (int16 bit patterns, any device) as a uint16 numpy array."""
    return depth16.cpu().numpy().view(np.uint16)


def render_path_frames(render_poses, hwf, K, chunk, render_kwargs, savedir=None, render_factor=0, seed=0):
    """run_plnerf.py:178-216 through plnerf_render_view: one library call per pose; returns (rgbs [n,H,W,3], disps [n,H,W])
    as numpy arrays, as render_path does.  Frame i draws under (seed, step = i): it is, bit for bit, what render() gives for
    that pose as a device tensor under DrawSource(seed, 0, i) (render_path under torch's own generator draws other numbers,
    and for host poses builds its rays with the host's arithmetic, an ulp away).  With `savedir`, frame i is also written as
    '{:03d}.png' of to8b(rgb): quantised on the device and copied to pinned host memory without blocking, two buffers deep,
    so encoding frame i overlaps rendering frame i + 1.  render_kwargs carries near / far / ndc as render() takes them."""
    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    H, W = int(H), int(W)
    kw = dict(render_kwargs)
    near, far, ndc = kw.pop("near", 0.), kw.pop("far", 1.), kw.pop("ndc", True)
    renderer = ViewRenderer(kw, H, W, K, chunk, near, far, ndc=ndc, seed=seed)
    n = len(render_poses)
    rgbs, disps = np.empty((n, H, W, 3), dtype=np.float32), np.empty((n, H, W), dtype=np.float32)
    if n == 0:
        return rgbs, disps
    if savedir is not None:
        os.makedirs(savedir, exist_ok=True)
    # host staging, two deep: frame i's copies are enqueued behind its render; they are waited for (and the PNG encoded)
    # after frame i + 1 has been enqueued
    stage = [{"rgb": torch.empty(H, W, 3).pin_memory(), "disp": torch.empty(H, W).pin_memory(),
              "rgb8": torch.empty(H, W, 3, dtype=torch.uint8).pin_memory(),
              "status": torch.zeros(2, dtype=torch.int32).pin_memory(), "done": torch.cuda.Event()} for _ in range(2)]
    # (the renderer has ONE set of planes: frame i + 1 overwrites them in stream order, after frame i's copies)

    def finish(i):
        s = stage[i % 2]
        s["done"].synchronize()
        renderer.check_range([int(b) for b in s["status"]])      # (render_path's check, on the words copied behind the frame)
        rgbs[i], disps[i] = s["rgb"].numpy(), s["disp"].numpy()
        if savedir is not None:
            write_png(os.path.join(savedir, '{:03d}.png'.format(i)), s["rgb8"].numpy())

    with torch.no_grad():
        for i, c2w in enumerate(render_poses):
            renderer.enqueue(torch.as_tensor(c2w)[:3, :4], step=i, export=savedir is not None)
            s = stage[i % 2]
            s["rgb"].copy_(renderer.planes["rgb"].view(H, W, 3), non_blocking=True)
            s["disp"].copy_(renderer.planes["disp"].view(H, W), non_blocking=True)
            if savedir is not None:
                s["rgb8"].copy_(renderer.rgb8.view(H, W, 3), non_blocking=True)
            for k, word in enumerate(renderer.status_words()):
                s["status"][k:k + 1].copy_(word, non_blocking=True)
            s["done"].record()
            if i > 0:
                finish(i - 1)
        finish(n - 1)
    return rgbs, disps
