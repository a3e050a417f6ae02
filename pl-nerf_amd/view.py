"""The host side of plnerf_render_view (include/plnerf_hip_view.h): one library call per rendered frame, and frames that
leave the device as 8-bit colour / 16-bit depth.

`ViewRenderer` owns what the call needs beyond the two networks -- the frame planes, the workspace the library carves up,
both packed weight buffers, the two linspace tables -- and the three structs of the ABI, filled once.  All of that is
onecall.Renderer's, which depthview.DepthViewRenderer stands on too; what is written here is this entry's own: which
configurations it serves, the pinhole camera in its config, and its two calls.  A frame is one
call: it packs both networks' weights, walks the view in blocks of `chunk` pixels and quantises the result on the
device.  What it computes is what render() computes under functional.DrawSource(seed, 0, step) for the same pose GIVEN AS A
DEVICE TENSOR, bit for bit: render() builds its rays with rays.get_rays where the pose lives, and the call's rays are the
device's evaluation of that expression.  (For a host pose render() takes the host's get_rays, whose directions differ from
the device's by an ulp; the frames then agree to rounding, not bit for bit.  The same holds for intrinsics whose focal lengths'
fp32 reciprocal 1.0f / float(f), which the call's rays multiply by, is not float(1.0 / f), which torch's device kernels multiply
by when get_rays divides by the Python float: 11.3, 9.7 and 1111.111 are one number either way, 10.77 is an ulp apart.
evaluate.entry_rays_are_renders(K) says which kind K is.)  Configurations outside the call (supported()) stay with render().

`render_path_frames` is render_path (run_plnerf.py:178-216) on that route, writing '{:03d}.png' per frame when asked to.
"""
import os

import numpy as np
import torch

from . import _lib as L
from .onecall import Renderer, fill_pinhole, fill_sampling, refusal_head
from .png import write_png
from .render import MAX_ROWS_PER_LAUNCH, _fusable


class ViewRenderer(Renderer):
    """Frames of H x W views through plnerf_render_view.  render_kwargs: create_nerf's dict (render_kwargs_test, say);
    K: the 3 x 3 intrinsics; chunk: pixels per block (render()'s chunk); near / far / ndc as render() takes them.  A frame
    is render()'s for a device-resident c2w under DrawSource(seed, 0, step), bit for bit (the module docstring has the
    condition); the pose handed to render() / enqueue() here may live anywhere, 12 host floats are read from it."""
    ENTRY, IO, ARGS, FALLBACK = "plnerf_render_view", L.ViewIo, L.ViewArgs, "render()"

    @staticmethod
    def unsupported_reason(render_kwargs):
        """Why plnerf_render_view cannot serve this configuration (None: it can)."""
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
        if c.precision != f.precision:
            return "both networks must run in one precision"
        for n in (c, f):
            if not (n.is_native() and n.density_beta == 0.0 and _fusable(n, emb[0], emb[1], True)):
                return "a network is outside the fused trunk with the in-kernel encoding and view directions"
            if not all(p.is_cuda for p in n.param_list()):
                return "the networks must live on the GPU"
        return None

    def __init__(self, render_kwargs, H, W, K, chunk, near, far, ndc=False, seed=0):
        kw = self._accepted(render_kwargs)
        cfg = L.StepConfig()
        constant = kw["mode"] == "constant" or bool(kw.get("constant_init", False))      # (run_plnerf.py:710-711)
        fill_sampling(cfg, kw, chunk, kw["network_fn"], seed, mode="constant" if constant else "linear")
        fill_pinhole(cfg, ndc, K, H, W, near, far)
        self._build(kw, cfg, H, W, far)

    def enqueue(self, c2w, step=0, export=False, pix0=0, n_pix=None):
        """Enqueue pixels [pix0, pix0 + n_pix) of the view `c2w` on the current stream (the whole view by default); nothing
        is synchronised.  The planes (self.planes, self.rgb8, self.depth16) hold the result once the stream gets there."""
        self._aim(c2w, step, export, pix0, n_pix)
        self._call()

    def render(self, c2w, step=0, export=False):
        """[rgb_map, disp_map, acc_map, extras] of the full view, shaped like render()'s result; every tensor is a view
        of this renderer's planes (valid until its next frame).  extras: rgb0, disp0, acc0, depth0, depth_map, z_std,
        and with export=True rgb8 [H,W,3] uint8 and depth16 [H,W] (int16 holding the uint16 codes of depth / far)."""
        with torch.no_grad():
            self.enqueue(c2w, step, export)
            self.check_range()
        return self._result(export)


def depth16_numpy(depth16):
    """ViewRenderer's depth16 plane (int16 bit patterns, any device) as a uint16 numpy array."""
    return depth16.cpu().numpy().view(np.uint16)


def render_path_frames(render_poses, hwf, K, chunk, render_kwargs, savedir=None, render_factor=0, seed=0,
                       max_net_rows=MAX_ROWS_PER_LAUNCH):
    """run_plnerf.py:178-216 through plnerf_render_view -- or, for a pair of networks that entry does not serve (one outside
    the fused trunk), through plnerf_render_view_any (anyview.AnyViewRenderer; max_net_rows bounds the rows one call of such
    a network takes, and with them the workspace) --: one library call per pose; returns (rgbs [n,H,W,3], disps [n,H,W])
    as numpy arrays, as render_path does.  Frame i draws under (seed, step = i): it is, bit for bit, what render() gives for
    that pose as a device tensor under DrawSource(seed, 0, i), for focal lengths as the module docstring describes them
    (render_path under torch's own generator draws other numbers, and for host poses builds its rays with the host's
    arithmetic, an ulp away).  With `savedir`, frame i is also written as
    '{:03d}.png' of to8b(rgb): quantised on the device and copied to pinned host memory without blocking, two buffers deep,
    so encoding frame i overlaps rendering frame i + 1.  render_kwargs carries near / far / ndc as render() takes them."""
    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    H, W = int(H), int(W)
    kw = dict(render_kwargs)
    near, far, ndc = kw.pop("near", 0.), kw.pop("far", 1.), kw.pop("ndc", True)
    from .anyview import frame_renderer      # (imported here: that module stands on this one)
    renderer = frame_renderer(kw, H, W, K, chunk, near, far, ndc=ndc, seed=seed, max_net_rows=max_net_rows)
    if renderer is None:      # (neither entry serves it: ViewRenderer's ValueError, as before)
        renderer = ViewRenderer(kw, H, W, K, chunk, near, far, ndc=ndc, seed=seed)
    n = len(render_poses)
    rgbs, disps = np.empty((n, H, W, 3), dtype=np.float32), np.empty((n, H, W), dtype=np.float32)
    if n == 0:
        return rgbs, disps
    export = savedir is not None
    copies = [("rgb", renderer.planes["rgb"].view(H, W, 3)), ("disp", renderer.planes["disp"].view(H, W))]
    if export:
        os.makedirs(savedir, exist_ok=True)
        copies.append(("rgb8", renderer.rgb8.view(H, W, 3)))      # (quantised on the device)

    def enqueue(i):
        renderer.enqueue(torch.as_tensor(render_poses[i])[:3, :4], step=i, export=export)

    def finish(i, s):      # (behind frame i + 1's enqueue: the PNG is encoded while that frame renders)
        rgbs[i], disps[i] = s["rgb"].numpy(), s["disp"].numpy()
        if export:
            write_png(os.path.join(savedir, '{:03d}.png'.format(i)), s["rgb8"].numpy())

    renderer.staged_frames(n, enqueue, copies, finish)
    return rgbs, disps
