"""What the host objects of the four one-call entries share -- stepplan.StepPlan / DepthStepPlan (plnerf_train_step,
plnerf_depth_train_step and their _const siblings) and view.ViewRenderer / depthview.DepthViewRenderer (plnerf_render_view,
plnerf_depth_render_view) -- written once, as include/plnerf_hip_onecall.cuh does for the entries themselves.

The config fillers are plain functions over a ctypes struct: a field of the C config structs that several entries carry is
written in ONE place here, from a tuple that the plans' keys are built from too (sampling(), pinhole()), so a key cannot go
stale against the config it describes.  They load no library and touch no device.  Then the aligned workspace, the two
linspace tables, and `Renderer`: all of a frame renderer that does not depend on which entry renders -- the buffers and
structs, current() / status_words() / check_range(), the pose and pixel range of a call, the shaped result, and the
two-deep staging loop that carries frames to the host.  No function here knows its caller: what differs between the
entries arrives as data (a struct class, an entry's name, a cap, a list of planes).
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import functional as Fn
from .nerf import NeRF


# ----------------------------------------------------------------------------- config fillers (host only)
def sampling(kw):
    """(n_samples, n_importance, color_mode, lindisp, perturb, white_bkgd, raw_noise_std, zero_tol, epsilon, farcolorfix)
    as the config structs hold them, from render kwargs.  N_samples and N_importance are required; the rest default to
    midpoint, 0, 0, 0, 0.0, 1e-4, 1e-3, 0."""
    return (int(kw["N_samples"]), int(kw["N_importance"]), L.COLOR[kw.get("color_mode", "midpoint")],
            int(bool(kw.get("lindisp", False))), int(kw.get("perturb", 0.) > 0.), int(bool(kw.get("white_bkgd", False))),
            float(kw.get("raw_noise_std", 0.)), float(kw.get("zero_tol", 1e-4)), float(kw.get("epsilon", 1e-3)),
            int(bool(kw.get("farcolorfix", False))))


def fill_sampling(cfg, kw, max_rays, coarse, seed, mode=None):
    """The fields every one-call config has: sampling(kw), the block size, what the kernels must know of the networks
    (`coarse` speaks for both) and the seed.  farcolorfix is written where the struct has it; mode where one is given."""
    (cfg.n_samples, cfg.n_importance, cfg.color_mode, cfg.lindisp, cfg.perturb, cfg.white_bkgd, cfg.raw_noise_std,
     cfg.zero_tol, cfg.epsilon, farcolorfix) = sampling(kw)
    if hasattr(cfg, "farcolorfix"):
        cfg.farcolorfix = farcolorfix
    if mode is not None:
        cfg.mode = L.MODE[mode]
    cfg.max_rays, cfg.seed = int(max_rays), int(seed)
    cfg.precision, cfg.fwd_kernel = L.PRECISION[coarse.precision], L.FWD_KERNEL
    cfg.input_ch, cfg.input_ch_views = int(coarse.input_ch), int(coarse.hip_view_ch)


def pinhole(ndc, K, H, W, near, far):
    """(ndc, ndc_focal, H, W, fx, fy, cx, cy, near, far) of plnerf_step_config."""
    return (int(bool(ndc)), float(K[0][0]), int(H), int(W), float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]),
            float(near), float(far))


def fill_pinhole(cfg, ndc, K, H, W, near, far):
    (cfg.ndc, cfg.ndc_focal, cfg.H, cfg.W, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.near, cfg.far) = pinhole(ndc, K, H, W, near, far)


def fill_depth(cfg, input_scale, coarse):
    """The depth variant's encoding scale and density activation."""
    cfg.input_scale, cfg.density_beta = float(input_scale), float(coarse.density_beta)


def fill_adam(cfg, group):
    """Adam's constants from an optimizer's parameter group."""
    cfg.beta1, cfg.beta2, cfg.adam_eps = float(group['betas'][0]), float(group['betas'][1]), float(group['eps'])


# ----------------------------------------------------------------------------- workspace and tables
def aligned_workspace(nbytes, device, zero=False):
    """An fp32 tensor of at least `nbytes` bytes whose address is a multiple of the workspace alignment."""
    raw = (torch.zeros if zero else torch.empty)((nbytes + L.STEP_WORKSPACE_ALIGN) // 4 + 1, device=device, dtype=torch.float32)
    pad = (-raw.data_ptr()) % L.STEP_WORKSPACE_ALIGN
    return raw[pad // 4:]


def tables(cfg, io, device):
    """The two linspace tables (t_vals, u_vals) of a config's sample counts, their addresses written into `io`."""
    t_vals, u_vals = Fn.cpu_linspace(cfg.n_samples, device), Fn.cpu_linspace(cfg.n_importance, device)
    io.t_vals, io.u_vals = t_vals.data_ptr(), u_vals.data_ptr()
    return t_vals, u_vals


# ----------------------------------------------------------------------------- frame renderers
def refusal_head(kw, max_samples, constant=False):
    """The refusals both frame renderers start with (None: none applies).  max_samples: the entry's cap on N_samples +
    N_importance; constant: the caller runs in piecewise-constant mode whatever kw["mode"] says."""
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
    if S < (3 if kw["mode"] == "constant" or constant else 2) or S + N > max_samples:
        return "the sample counts are outside the kernels' limits"
    return None


class Renderer:
    """Frames of H x W views through one library call each.  A subclass names its entry and its structs, fills a config
    and hands it to _build(); what a frame needs beyond the pose and the pixel range it writes in its own enqueue()."""
    ENTRY = None         # the entry point; ENTRY + "_workspace_bytes" sizes its workspace
    IO = ARGS = None     # the ctypes mirrors of the entry's io and args structs
    FALLBACK = None      # the multi-call route a refusal points to

    @classmethod
    def supported(cls, render_kwargs):
        return cls.unsupported_reason(render_kwargs) is None

    def _accepted(self, render_kwargs):
        why = self.unsupported_reason(render_kwargs)
        if why is not None:
            raise ValueError(f"{type(self).__name__}: {why}; use {self.FALLBACK}")
        return render_kwargs

    def _build(self, kw, cfg, H, W, far):
        """Everything behind a filled config: the workspace, the tables, the frame planes, both packed buffers and the io /
        args structs."""
        self.nets = (kw["network_fn"], kw["network_fine"])
        dev = next(self.nets[0].parameters()).device
        self.device, self.H, self.W, self.far = dev, int(H), int(W), float(far)
        self.precision = self.nets[0].precision
        self.config = cfg
        io = self.io = self.IO()
        self._bind_networks()      # (ahead of the size query: an entry may size its workspace by what the slots hold)
        nbytes = self._workspace_bytes()
        if nbytes == 0:
            raise ValueError(f"{type(self).__name__}: {self.ENTRY} refuses this configuration; use {self.FALLBACK}")
        self.workspace, self.workspace_bytes = aligned_workspace(nbytes, dev), nbytes
        self.t_vals, self.u_vals = tables(cfg, io, dev)
        n = self.H * self.W
        self.planes = {name: torch.empty((n, 3) if name in ("rgb", "rgb0") else (n,), device=dev) for name in L.VIEW_PLANES}
        self.rgb8 = torch.empty(n, 3, device=dev, dtype=torch.uint8)
        self.depth16 = torch.empty(n, device=dev, dtype=torch.int16)      # (uint16 bit patterns: depth / far)
        for name in L.VIEW_PLANES:
            setattr(io, name, self.planes[name].data_ptr())
        self.args = self.ARGS()
        self.args.pack_weights = 1
        self.args.depth16_scale = float(np.float32(1.0) / np.float32(far))
        self._refs = (ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(self.args), ctypes.c_void_p(self.workspace.data_ptr()))

    def _workspace_bytes(self):
        """The entry's size query (0: the configuration is refused)."""
        return getattr(L.lib(), self.ENTRY + "_workspace_bytes")(ctypes.byref(self.config))

    def _bind_networks(self):
        """Both networks into the io struct: two networks of the compiled trunk, their 24 parameter tensors each and the
        renderer's own packed buffers (zeroed once: the kernels only ever OR into the status word)."""
        cfg, io, dev = self.config, self.io, self.device
        packed_bytes = L.lib().plnerf_mlp_packed_bytes(cfg.precision)
        self.packed = tuple(torch.zeros(packed_bytes // 4, device=dev, dtype=torch.float32) for _ in range(2))
        self._status_off = L.lib().plnerf_mlp_status_offset(cfg.precision) // 4
        self._params = tuple([p.detach() for p in net.param_list()] for net in self.nets)
        for io_net, params, packed in zip((io.coarse, io.fine), self._params, self.packed):
            for k, p in enumerate(params):
                io_net.params[k] = L.dptr(p, f"params[{k}]").value
            io_net.packed = packed.data_ptr()

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
        """The rendering loops' check for the guarded precisions: a clamped frame must not pass silently.  bits: the two
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

    def _aim(self, c2w, step, export, pix0, n_pix):
        """The part of a call every entry takes: the pose (12 host floats are read from it), the step, the pixel range
        and whether the 8 / 16-bit planes are written.  Refuses a renderer whose networks have moved."""
        if not self.current():
            name = type(self).__name__
            raise RuntimeError(f"{name}: the networks' parameters moved; build a new {name}")
        a = self.args
        a.c2w[:] = [float(v) for v in torch.as_tensor(c2w, device="cpu")[:3, :4].reshape(-1)]
        a.step, a.pix0 = int(step), int(pix0)
        a.n_pix = self.H * self.W - int(pix0) if n_pix is None else int(n_pix)
        self.io.rgb8 = self.rgb8.data_ptr() if export else None
        self.io.depth16 = self.depth16.data_ptr() if export else None

    def _call(self):
        cfg, io, args, ws = self._refs
        L.check(getattr(L.lib(), self.ENTRY)(cfg, io, args, ws, self.workspace_bytes, L.stream()), self.ENTRY)

    def _result(self, export):
        """[rgb_map, disp_map, acc_map, extras] over the planes, shaped [H, W(, 3)]."""
        H, W = self.H, self.W
        shaped = {k: (v.view(H, W, 3) if v.dim() == 2 else v.view(H, W)) for k, v in self.planes.items()}
        extras = {"rgb0": shaped["rgb0"], "disp0": shaped["disp0"], "acc0": shaped["acc0"], "depth0": shaped["depth0"],
                  "depth_map": shaped["depth"], "z_std": shaped["z_std"]}
        if export:
            extras["rgb8"], extras["depth16"] = self.rgb8.view(H, W, 3), self.depth16.view(H, W)
        return [shaped["rgb"], shaped["disp"], shaped["acc"], extras]

    def staged_frames(self, n, enqueue, copies, finish):
        """Frames 0 .. n - 1 to the host, two pinned buffers deep: enqueue(i) enqueues frame i; `copies`, pairs of (stage
        key, device tensor), are then copied behind it without blocking, the status words with them; they are waited for,
        the words checked and finish(i, stage) called after frame i + 1 has been enqueued, so the host's work on a frame
        overlaps the next one's rendering.  (The renderer has ONE set of planes: frame i + 1 overwrites them in stream
        order, after frame i's copies.)"""
        stage = [dict({key: torch.empty(src.shape, dtype=src.dtype).pin_memory() for key, src in copies},
                      status=torch.zeros(2, dtype=torch.int32).pin_memory(), done=torch.cuda.Event()) for _ in range(2)]

        def done(i):
            s = stage[i % 2]
            s["done"].synchronize()
            self.check_range([int(b) for b in s["status"]])      # (on the words copied behind the frame)
            finish(i, s)

        with torch.no_grad():
            for i in range(n):
                enqueue(i)
                s = stage[i % 2]
                for key, src in copies:
                    s[key].copy_(src, non_blocking=True)
                for k, word in enumerate(self.status_words()):
                    if word is not None:      # (a network without a status word: its entry of the pair stays 0)
                        s["status"][k:k + 1].copy_(word, non_blocking=True)
                s["done"].record()
                if i > 0:
                    done(i - 1)
            done(n - 1)
