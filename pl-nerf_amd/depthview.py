"""The host side of plnerf_depth_render_view (include/experimental/plnerf_hip_depthview.h): one library call per rendered
frame of the depth-supervised variant (depth.py), its `test_samples_error` row scored while the hypotheses are in the
workspace, and frames that leave the device as 8-bit colour / 16-bit depth.

`DepthViewRenderer` is view.ViewRenderer for that variant, on the same base (onecall.Renderer owns the frame planes, the
workspace, both packed weight buffers, the two linspace tables and the three structs of the (experimental) ABI, filled
once); what is written here is this entry's own: the per-call intrinsic, the hypothesis plane, the sampling-error row and
the millimetre plane.  What a frame holds is what
depth.render() computes under functional.DrawSource(seed, 0, step) for the same pose and intrinsics GIVEN AS DEVICE TENSORS,
bit for bit: depth.render() builds its rays with depth.get_rays where the pose lives, and the call's rays are the device's
evaluation of those expressions.  Configurations outside the call (supported()) stay with depth.render().

`render_video_frames` is the frame loop of render_video (run_nerf_sample_based_depth.py:277-295) on that route: '{idx}.png'
of to8b(rgb) and of the depth in millimetres, without the colour-mapped plane and without the mp4.
"""
import os

import numpy as np
import torch

from . import _lib as L
from .onecall import Renderer, fill_depth, fill_sampling, refusal_head
from .png import write_png


class DepthViewRenderer(Renderer):
    """Frames of H x W views through plnerf_depth_render_view.  render_kwargs: depth.create_nerf's dict (render_kwargs_test,
    say) without near / far; chunk: pixels per block (depth.render()'s chunk).  The pose and the intrinsic (fx, fy, cx, cy)
    handed to render() / enqueue() may live anywhere: 12 + 4 host floats are read from them."""
    ENTRY, IO, ARGS, FALLBACK = "plnerf_depth_render_view", L.DepthViewIo, L.DepthViewArgs, "depth.render()"

    @staticmethod
    def unsupported_reason(render_kwargs):
        """Why plnerf_depth_render_view cannot serve this configuration (None: it can)."""
        from .depth import _host_box, _kernel_encoding
        kw = render_kwargs
        why = refusal_head(kw, L.DEPTH_STEP_MAX_SAMPLES)
        if why is not None:
            return why
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
        c, f = kw["network_fn"], kw["network_fine"]
        if c.precision != f.precision or c.density_beta != f.density_beta:
            return "both networks must run in one precision and with one density activation"
        for n in (c, f):
            if not (n.is_native() and n.has_fused_encoding() and n.input_ch == 3 + 6 * enc[0] and
                    n.input_ch_views == 3 + 6 * enc[1]):
                return "a network is outside the fused trunk with the in-kernel encoding and view directions"
            if not all(p.is_cuda for p in n.param_list()):
                return "the networks must live on the GPU"
        return None

    def __init__(self, render_kwargs, H, W, chunk, near, far, seed=0):
        from .depth import _kernel_encoding
        kw = self._accepted(render_kwargs)
        coarse = kw["network_fn"]
        cfg = L.DepthViewConfig()
        fill_sampling(cfg, kw, chunk, coarse, seed, mode=kw["mode"])
        cfg.H, cfg.W, cfg.near, cfg.far = int(H), int(W), float(near), float(far)
        emb = kw["network_query_fn"].embedders
        fill_depth(cfg, _kernel_encoding(emb[0], emb[1], True)[2], coarse)
        self._build(kw, cfg, H, W, far)
        self._pred_hyp = None                                                 # [H W, N], allocated when first asked for
        self.error_row = torch.zeros(L.SAMPLEERR_ROW, dtype=torch.float64, device=self.device)
        self.depth_mm16 = torch.empty(self.H * self.W, device=self.device, dtype=torch.int16)      # (uint16 bit patterns: millimetres)
        self.args.depth_mm_mult = 1000.0
        self._valid = None

    @property
    def pred_hyp(self):
        """The hypothesis plane [H W, n_importance] (allocated on first use: a frame that is only scored never has one)."""
        if self._pred_hyp is None:
            self._pred_hyp = torch.empty(self.H * self.W, self.config.n_importance, device=self.device)
        return self._pred_hyp

    def enqueue(self, c2w, intrinsic, step=0, export=False, pix0=0, n_pix=None, valid=None, want_hyp=False):
        """Enqueue pixels [pix0, pix0 + n_pix) of the view (c2w, intrinsic = (fx, fy, cx, cy)) on the current stream (the
        whole view by default); nothing is synchronised.  valid: [H W] (any shape) of the pixels the sampling error counts;
        every block then ADDS its two values to self.error_row, which the caller zeroes before a frame's first call
        (render() does).  want_hyp: also keep the hypotheses (self.pred_hyp).  The planes hold the result once the stream
        gets there.  The call reads 12 + 4 HOST floats: hand over host tensors (or lists) and nothing waits for the device; a
        pose or an intrinsic that lives on the device costs a blocking device-to-host copy each, per call -- a loop over many
        views copies them to the host once, before it starts (as depth.test_images_samples(one_call=True) does)."""
        self._aim(c2w, step, export, pix0, n_pix)
        a, io = self.args, self.io
        a.fx, a.fy, a.cx, a.cy = [float(v) for v in torch.as_tensor(intrinsic, device="cpu").reshape(-1)[:4]]
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
        self._call()

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
        ret = self._result(export)
        extras = ret[3]
        if want_hyp:
            extras["pred_hyp"] = self.pred_hyp.view(self.H, self.W, -1)
        if valid is not None:
            extras["sample_error_row"] = self.error_row
        if export:
            extras["depth_mm16"] = self.depth_mm16.view(self.H, self.W)
        return ret


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

    def finish(i, s):
        write_png(os.path.join(rgb_dir, frame_name(i)), s["rgb8"].numpy())
        write_png(os.path.join(depth_dir, frame_name(i)), s["mm16"].numpy().view(np.uint16))

    renderer.staged_frames(n, lambda i: renderer.enqueue(host_poses[i], intr[i], step=i, export=True),
                           [("rgb8", renderer.rgb8.view(H, W, 3)), ("mm16", renderer.depth_mm16.view(H, W))], finish)
    return n


def frame_name(idx):
    """render_video's file name of frame idx (:293-294: str(img_idx) + '.png', no zero padding)."""
    return '{}.png'.format(idx)
