"""The host side of plnerf_depth_render_view (include/experimental/plnerf_hip_depthview.h): one library call per rendered
frame of the depth-supervised variant (depth.py), its `test_samples_error` row scored while the hypotheses are in the
workspace, and frames that leave the device as 8-bit colour / 16-bit depth.

`DepthViewRenderer` is view.ViewRenderer for that variant: it owns the frame planes, the workspace, both packed weight
buffers, the two linspace tables and the three structs of the (experimental) ABI, filled once.  What a frame holds is what
depth.render() computes under functional.DrawSource(seed, 0, step) for the same pose and intrinsics GIVEN AS DEVICE TENSORS,
bit for bit: depth.render() builds its rays with depth.get_rays where the pose lives, and the call's rays are the device's
evaluation of those expressions.  Configurations outside the call (supported()) stay with depth.render().

`render_video_frames` is the frame loop of render_video (run_nerf_sample_based_depth.py:277-295) on that route: '{idx}.png'
of to8b(rgb) and of the depth in millimetres, without the colour-mapped plane and without the mp4.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from . import functional as Fn
from .nerf import NeRF
from .png import write_png
from .view import _aligned


class DepthViewRenderer:
    """Frames of H x W views through plnerf_depth_render_view.  render_kwargs: depth.create_nerf's dict (render_kwargs_test,
    say) without near / far; chunk: pixels per block (depth.render()'s chunk).  The pose and the intrinsic (fx, fy, cx, cy)
    handed to render() / enqueue() may live anywhere: 12 + 4 host floats are read from them."""

    @staticmethod
    def unsupported_reason(render_kwargs):
        """Why plnerf_depth_render_view cannot serve this configuration (None: it can)."""
        from .depth import _host_box, _kernel_encoding
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
        if S < (3 if kw["mode"] == "constant" else 2) or S + N > L.DEPTH_STEP_MAX_SAMPLES:
            return "the sample counts are outside the kernels' limits"
        if kw.get("is_joint", False):
            return "is_joint stays with depth.render()"
        if kw.get("pytest", False) or kw.get("retraw", False) or kw.get("c2w_staticcam") is not None or kw.get("with_5_9", False):
            return "pytest draws, retraw, with_5_9 and c2w_staticcam stay with depth.render()"
        if kw.get("precomputed_z_samples") is not None or kw.get("cached_u") is not None:
            return "precomputed samples and cached draws stay with depth.render()"
        cam = kw.get("embedded_cam")
        if cam is not None and cam.numel() > 0:
            return "a camera code (embedded_cam) stays with depth.render()"
        qfn = kw.get("network_query_fn")
        emb, box = getattr(qfn, "embedders", None), getattr(qfn, "box", None)      # (create_nerf's query function says them)
        if emb is None or box is None:
            return "network_query_fn does not name its encoders and its box (depth.create_nerf's does)"
        enc = _kernel_encoding(emb[0], emb[1], True)
        if enc is None or not _host_box(*box)[2]:
            return "the in-kernel encoding needs the package's encoders and an identity bounding box"
        if c.precision != f.precision or c.density_beta != f.density_beta:
            return "both networks must run in one precision and with one density activation"
        for n in (c, f):
            if not (n.is_native() and n.has_fused_encoding() and n.input_ch == 3 + 6 * enc[0] and
                    n.input_ch_views == 3 + 6 * enc[1]):
                return "a network is outside the fused trunk with the in-kernel encoding and view directions"
            if not all(p.is_cuda for p in n.param_list()):
                return "the networks must live on the GPU"
        return None

    @staticmethod
    def supported(render_kwargs):
        return DepthViewRenderer.unsupported_reason(render_kwargs) is None

    def __init__(self, render_kwargs, H, W, chunk, near, far, seed=0):
        from .depth import _kernel_encoding
        why = self.unsupported_reason(render_kwargs)
        if why is not None:
            raise ValueError(f"DepthViewRenderer: {why}; use depth.render()")
        kw = render_kwargs
        self.nets = (kw["network_fn"], kw["network_fine"])
        coarse = self.nets[0]
        dev = coarse.param_list()[0].device
        self.device, self.H, self.W, self.far = dev, int(H), int(W), float(far)
        self.precision = coarse.precision
        cfg = self.config = L.DepthViewConfig()
        cfg.max_rays, cfg.n_samples, cfg.n_importance = int(chunk), int(kw["N_samples"]), int(kw["N_importance"])
        cfg.mode, cfg.color_mode = L.MODE[kw["mode"]], L.COLOR[kw.get("color_mode", "midpoint")]
        cfg.lindisp, cfg.perturb = int(bool(kw.get("lindisp", False))), int(kw.get("perturb", 0.) > 0.)
        cfg.white_bkgd = int(bool(kw.get("white_bkgd", False)))
        cfg.raw_noise_std = float(kw.get("raw_noise_std", 0.))
        cfg.zero_tol, cfg.epsilon = float(kw.get("zero_tol", 1e-4)), float(kw.get("epsilon", 1e-3))
        cfg.H, cfg.W, cfg.near, cfg.far = int(H), int(W), float(near), float(far)
        cfg.precision, cfg.fwd_kernel = L.PRECISION[coarse.precision], L.FWD_KERNEL
        cfg.input_ch, cfg.input_ch_views = int(coarse.input_ch), int(coarse.hip_view_ch)
        emb = kw["network_query_fn"].embedders
        cfg.input_scale, cfg.density_beta = float(_kernel_encoding(emb[0], emb[1], True)[2]), float(coarse.density_beta)
        cfg.seed = int(seed)
        nbytes = L.lib().plnerf_depth_render_view_workspace_bytes(ctypes.byref(cfg))
        if nbytes == 0:
            raise ValueError("DepthViewRenderer: plnerf_depth_render_view refuses this configuration; use depth.render()")
        self.workspace, self.workspace_bytes = _aligned(nbytes, dev), nbytes
        self.t_vals = Fn.cpu_linspace(cfg.n_samples, dev)
        self.u_vals = Fn.cpu_linspace(cfg.n_importance, dev)
        n = self.H * self.W
        self.planes = {name: torch.empty((n, 3) if name in ("rgb", "rgb0") else (n,), device=dev) for name in L.VIEW_PLANES}
        self._pred_hyp = None                                                 # [H W, N], allocated when first asked for
        self.error_row = torch.zeros(L.SAMPLEERR_ROW, dtype=torch.float64, device=dev)
        self.rgb8 = torch.empty(n, 3, device=dev, dtype=torch.uint8)
        self.depth16 = torch.empty(n, device=dev, dtype=torch.int16)          # (uint16 bit patterns: depth / far)
        self.depth_mm16 = torch.empty(n, device=dev, dtype=torch.int16)       # (uint16 bit patterns: millimetres)
        # the renderer's own packed buffers (zeroed once: the kernels only ever OR into the status word)
        packed_bytes = L.lib().plnerf_mlp_packed_bytes(cfg.precision)
        self.packed = tuple(torch.zeros(packed_bytes // 4, device=dev, dtype=torch.float32) for _ in range(2))
        self._status_off = L.lib().plnerf_mlp_status_offset(cfg.precision) // 4
        io = self.io = L.DepthViewIo()
        self._params = tuple([p.detach() for p in net.param_list()] for net in self.nets)
        for io_net, params, packed in zip((io.coarse, io.fine), self._params, self.packed):
            for k, p in enumerate(params):
                io_net.params[k] = L.dptr(p, f"params[{k}]").value
            io_net.packed = packed.data_ptr()
        io.t_vals, io.u_vals = self.t_vals.data_ptr(), self.u_vals.data_ptr()
        for name in L.VIEW_PLANES:
            setattr(io, name, self.planes[name].data_ptr())
        self.args = L.DepthViewArgs()
        self.args.pack_weights = 1
        self.args.depth16_scale = float(np.float32(1.0) / np.float32(far))
        self.args.depth_mm_mult = 1000.0
        self._valid = None
        self._refs = (ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(self.args), ctypes.c_void_p(self.workspace.data_ptr()))

    @property
    def pred_hyp(self):
        """The hypothesis plane [H W, n_importance] (allocated on first use: a frame that is only scored never has one)."""
        if self._pred_hyp is None:
            self._pred_hyp = torch.empty(self.H * self.W, self.config.n_importance, device=self.device)
        return self._pred_hyp

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
        """The evaluation loops' check for the guarded precisions: a clamped frame must not pass silently.  bits: the two
        status words as host integers (a caller that copied them itself); None reads them from the device (synchronises)."""
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

    def enqueue(self, c2w, intrinsic, step=0, export=False, pix0=0, n_pix=None, valid=None, want_hyp=False):
        """Enqueue pixels [pix0, pix0 + n_pix) of the view (c2w, intrinsic = (fx, fy, cx, cy)) on the current stream (the
        whole view by default); nothing is synchronised.  valid: [H W] (any shape) of the pixels the sampling error counts;
        every block then ADDS its two values to self.error_row, which the caller zeroes before a frame's first call
        (render() does).  want_hyp: also keep the hypotheses (self.pred_hyp).  The planes hold the result once the stream
        gets there.  The call reads 12 + 4 HOST floats: hand over host tensors (or lists) and nothing waits for the device; a
        pose or an intrinsic that lives on the device costs a blocking device-to-host copy each, per call -- a loop over many
        views copies them to the host once, before it starts (as depth.test_images_samples(one_call=True) does)."""
        if not self.current():
            raise RuntimeError("DepthViewRenderer: the networks' parameters moved; build a new DepthViewRenderer")
        a = self.args
        a.c2w[:] = [float(v) for v in torch.as_tensor(c2w, device="cpu")[:3, :4].reshape(-1)]
        a.fx, a.fy, a.cx, a.cy = [float(v) for v in torch.as_tensor(intrinsic, device="cpu").reshape(-1)[:4]]
        a.step, a.pix0 = int(step), int(pix0)
        a.n_pix = self.H * self.W - int(pix0) if n_pix is None else int(n_pix)
        io = self.io
        io.rgb8 = self.rgb8.data_ptr() if export else None
        io.depth16 = self.depth16.data_ptr() if export else None
        io.depth_mm16 = self.depth_mm16.data_ptr() if export else None
        io.pred_hyp = self.pred_hyp.data_ptr() if want_hyp else None
        if valid is not None:
            valid = torch.as_tensor(valid).to(device=self.device).ne(0).to(torch.uint8).reshape(-1).contiguous()
            if valid.numel() != self.H * self.W:
                raise ValueError(f"valid must hold H W = {self.H * self.W} values, got {valid.numel()}")
            io.valid, io.error_row = valid.data_ptr(), self.error_row.data_ptr()
        else:
            io.valid, io.error_row = None, None
        self._valid = valid      # (alive until the next call is enqueued behind this one)
        cfg, io_ref, args, ws = self._refs
        L.check(L.lib().plnerf_depth_render_view(cfg, io_ref, args, ws, self.workspace_bytes, L.stream()),
                "plnerf_depth_render_view")

    def render(self, c2w, intrinsic, step=0, export=False, valid=None, want_hyp=False, check=True):
        """[rgb_map, disp_map, acc_map, extras] of the full view, shaped like depth.render()'s result; every tensor is a
        view of this renderer's planes (valid until its next frame).  extras: rgb0, disp0, acc0, depth0, depth_map, z_std;
        with want_hyp pred_hyp [H,W,N]; with `valid` sample_error_row (fp64 [2]: the sum over the valid pixels of
        mean_k |pred_hyp - depth| and their number); with export=True rgb8 [H,W,3] uint8, depth16 and depth_mm16 [H,W]
        (int16 holding the uint16 codes of depth / far and of the depth in millimetres).  check: read the range status words
        behind the frame (check_range(): a host synchronisation per frame); a loop passes False and calls check_range() once
        after its last frame -- the words are sticky."""
        with torch.no_grad():
            if valid is not None:
                self.error_row.zero_()
            self.enqueue(c2w, intrinsic, step, export, valid=valid, want_hyp=want_hyp)
            if check:
                self.check_range()
        H, W, p = self.H, self.W, self.planes
        shaped = {k: (v.view(H, W, 3) if v.dim() == 2 else v.view(H, W)) for k, v in p.items()}
        extras = {"rgb0": shaped["rgb0"], "disp0": shaped["disp0"], "acc0": shaped["acc0"], "depth0": shaped["depth0"],
                  "depth_map": shaped["depth"], "z_std": shaped["z_std"]}
        if want_hyp:
            extras["pred_hyp"] = self.pred_hyp.view(H, W, -1)
        if valid is not None:
            extras["sample_error_row"] = self.error_row
        if export:
            extras["rgb8"], extras["depth16"] = self.rgb8.view(H, W, 3), self.depth16.view(H, W)
            extras["depth_mm16"] = self.depth_mm16.view(H, W)
        return [shaped["rgb"], shaped["disp"], shaped["acc"], extras]


def render_video_frames(poses, H, W, intrinsics, rgb_dir, depth_dir, render_kwargs_test, chunk, seed=0):
    """The frame loop of render_video (run_nerf_sample_based_depth.py:277-295) through plnerf_depth_render_view: one library
    call per pose.  Frame idx is written as '{idx}.png' of to8b(rgb) under rgb_dir and of (depth * 1000) as uint16 under
    depth_dir, both quantised on the device (5 bytes per pixel leave it) and copied to pinned host memory without blocking,
    two buffers deep, so encoding frame idx overlaps rendering frame idx + 1.  The colour-mapped depth plane and the mp4 are
    not written.  intrinsics: one (fx, fy, cx, cy) for every pose, or [n, 4]; render_kwargs_test carries near / far as
    depth.render() takes them.  Frame idx draws under (seed, step = idx).  Returns the number of frames written."""
    H, W = int(H), int(W)
    kw = dict(render_kwargs_test)
    near, far = kw.pop("near", 0.), kw.pop("far", 1.)
    kw.pop("ndc", None)      # (accepted and unused by depth.render())
    renderer = DepthViewRenderer(kw, H, W, chunk, near, far, seed=seed)
    n = len(poses)
    if n == 0:
        return 0
    os.makedirs(rgb_dir, exist_ok=True)
    os.makedirs(depth_dir, exist_ok=True)
    intr = torch.as_tensor(intrinsics, device="cpu").float()
    intr = intr.reshape(1, 4).expand(n, 4) if intr.numel() == 4 else intr.reshape(n, -1)
    # (host copies, made once: enqueue reads host floats and must not wait for the device between two frames)
    host_poses = [torch.as_tensor(c2w).detach().to(device="cpu", dtype=torch.float32)[:3, :4] for c2w in poses]
    stage = [{"rgb8": torch.empty(H, W, 3, dtype=torch.uint8).pin_memory(),
              "mm16": torch.empty(H, W, dtype=torch.int16).pin_memory(),
              "status": torch.zeros(2, dtype=torch.int32).pin_memory(), "done": torch.cuda.Event()} for _ in range(2)]
    # (the renderer has ONE set of planes: frame idx + 1 overwrites them in stream order, after frame idx's copies)

    def finish(i):
        s = stage[i % 2]
        s["done"].synchronize()
        renderer.check_range([int(b) for b in s["status"]])
        write_png(os.path.join(rgb_dir, frame_name(i)), s["rgb8"].numpy())
        write_png(os.path.join(depth_dir, frame_name(i)), s["mm16"].numpy().view(np.uint16))

    with torch.no_grad():
        for i, c2w in enumerate(host_poses):
            renderer.enqueue(c2w, intr[i], step=i, export=True)
            s = stage[i % 2]
            s["rgb8"].copy_(renderer.rgb8.view(H, W, 3), non_blocking=True)
            s["mm16"].copy_(renderer.depth_mm16.view(H, W), non_blocking=True)
            for k, word in enumerate(renderer.status_words()):
                s["status"][k:k + 1].copy_(word, non_blocking=True)
            s["done"].record()
            if i > 0:
                finish(i - 1)
        finish(n - 1)
    return n


def frame_name(idx):
    """render_video's file name of frame idx (:293-294: str(img_idx) + '.png', no zero padding)."""
    return '{}.png'.format(idx)
