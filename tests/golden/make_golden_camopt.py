"""Generate tests/golden/g10_camera_code_opt.npz from the REFERENCE itself: its own optimize_camera_embedding
(depth_supervised_exps/run_nerf_sample_based_depth.py:311-347) run on the CPU, where `.to(device)` is the identity and the
loop runs as written.

Run in the build container only (make_golden.py's helpers import the reference read-only):

    python tests/golden/make_golden_camopt.py

The scene (tests/camopt_fp64.py restates it from the fixture's arrays): a 4 x 6 view, 8 + 8 samples, mode linear / midpoint,
white background, N_rand = 6 -- two batches of 12 pixels, and with equal sizes the objective does not depend on which pixels
random_split puts into which batch -- and input_ch_cam = 4.  Weights: the closed-form depth recipe (seeds 0 and 1, sharpened),
the four extra view-layer columns of each network from a closed-form sine, as G8c's (stored: they are not part of the recipe).
The target is the same scene rendered at a non-zero code.

Recorded per iteration: the code before the step, the loss sum (the fp32 sum of the two batches' img2mse, as :328-339
accumulate it), the gradient Adam.step sees, the learning rate it uses and the PSNR handed to the scheduler -- a 100-step
trajectory at lr 0.5 through ReLU kinks is not comparable across arithmetics, so the tests check every iteration on its own
from the recorded code -- and the final best code and best PSNR.  The installed torch's ReduceLROnPlateau has no `verbose`
keyword: a stand-in drops it.

H4: with perturb = 0 the importance draw is linspace(0, 1), and at u == 1 the reference's piecewise-linear sampler
indexes one past tau_diff (model/run_nerf_helpers.py:573) and raises on the CPU.  The generator runs the reference under a
torch.gather of its own that clamps the index to the axis -- what the oracle and the kernels define at that point
(oracle.plnerf_oracle.sample_pdf_reformulation) -- and is otherwise torch's."""
import os
import sys
from argparse import Namespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (imports the reference)
from make_golden import orc  # noqa: E402

H, W, NS, NI, N_RAND, N_CAM = 4, 6, 8, 8, 6, 4
NEAR, FAR = 2.0, 6.0
INTRINSIC = (5.0, 5.0, 3.0, 2.0)
CAM_TARGET = (0.8, -0.6, 0.5, -0.9)
EXTRA_AMPLITUDE = 1.5
SUBSET_CASES = ((24, 6), (24, 5), (24, 100), (100, 7), (101, 10), (1000, 32), (1023, 64), (12288, 1024), (292032, 1024),
                (292032, 4096), (7, 1), (97, 3))


def view_weight_extra(seed):
    idx = torch.arange(128 * N_CAM, dtype=torch.float64).reshape(128, N_CAM)
    return (EXTRA_AMPLITUDE * torch.sin(0.37 * idx + 1.3 + seed)).float()


class clamped_gather:
    """torch.gather with its index clamped to the axis, while the block runs (H4, above)."""

    def __enter__(self):
        self.gather = gather = torch.gather

        def clamped(input, dim, index, **kwargs):
            return gather(input, dim, index.clamp(max=input.shape[dim] - 1), **kwargs)
        torch.gather = clamped

    def __exit__(self, *exc):
        torch.gather = self.gather


def main():
    D, DH = MG.import_depth_reference()
    if not hasattr(D, "create_random_subsets"):      # (the script calls it at :323 without importing it: the reference's own)
        from data.dataset_sampling import create_random_subsets
        D.create_random_subsets = create_random_subsets
    embed_fn, input_ch = DH.get_embedder(9, 0)
    embeddirs_fn, input_ch_views = DH.get_embedder(0, 0)
    extras = [view_weight_extra(seed) for seed in (0, 1)]

    def net(seed):
        m = DH.NeRF(D=8, W=256, input_ch=input_ch, output_ch=5, skips=[4], input_ch_views=input_ch_views, input_ch_cam=N_CAM,
                    use_viewdirs=True)
        sd = orc.closed_form_state_dict_depth(seed, sharpen=True)
        sd["views_linears.0.weight"] = torch.cat([sd["views_linears.0.weight"], extras[seed]], 1)
        m.load_state_dict(sd)
        return m.requires_grad_(False)
    coarse, fine = net(0), net(1)

    def query(inputs, viewdirs, embedded_cam, fn):
        return D.run_network(inputs, viewdirs, embedded_cam, fn, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, bb_center=0.0,
                             bb_scale=1.0, netchunk=65536)
    kw = dict(network_query_fn=query, perturb=False, N_importance=NI, network_fine=fine, N_samples=NS, network_fn=coarse,
              use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint", near=NEAR, far=FAR,
              lindisp=False)
    args = Namespace(input_ch_cam=N_CAM, N_rand=N_RAND, chunk=1024)
    pose = orc.pose_spherical(30.0, -30.0, 4.0)[:3, :4].float()
    intrinsic = torch.tensor(INTRINSIC)
    with torch.no_grad(), clamped_gather():
        kw["embedded_cam"] = torch.tensor(CAM_TARGET)
        image = D.render(H, W, intrinsic, chunk=args.chunk, c2w=pose, **kw)[0]
        kw["embedded_cam"] = torch.zeros(N_CAM)
        rgb_zero = D.render(H, W, intrinsic, chunk=args.chunk, c2w=pose, **kw)[0]

    rec = {"cam": [], "grad": [], "lr": [], "psnr": [], "loss": []}
    adam_step, img2mse = torch.optim.Adam.step, D.img2mse
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau

    def step(self, closure=None):
        p = self.param_groups[0]["params"][0]
        rec["cam"].append(p.detach().clone())
        rec["grad"].append(p.grad.detach().clone())
        rec["lr"].append(float(self.param_groups[0]["lr"]))
        return adam_step(self, closure)

    def recorded_mse(x, y):
        out = img2mse(x, y)
        rec["loss"].append(out.detach().clone())
        return out

    class Plateau(plateau):      # the stand-in: drops `verbose`, records the metric
        def __init__(self, optimizer, mode="min", verbose=None, **kwargs):
            super().__init__(optimizer, mode, **kwargs)

        def step(self, metrics, *a, **k):
            rec["psnr"].append(torch.as_tensor(metrics).detach().reshape(()).clone())
            return super().step(metrics, *a, **k)

    torch.optim.Adam.step, D.img2mse, torch.optim.lr_scheduler.ReduceLROnPlateau = step, recorded_mse, Plateau
    try:
        with clamped_gather():
            D.optimize_camera_embedding(image, pose, H, W, intrinsic, args, kw)
    finally:
        torch.optim.Adam.step, D.img2mse, torch.optim.lr_scheduler.ReduceLROnPlateau = adam_step, img2mse, plateau
    n = len(rec["cam"])
    per = len(rec["loss"]) // n
    assert n == 100 and per == 2 and len(rec["loss"]) == per * n, (n, len(rec["loss"]))
    loss_sum = []
    for i in range(n):      # :328, :339: torch.zeros(1), += every batch's loss
        s = torch.zeros(1)
        for b in range(per):
            s += rec["loss"][i * per + b]
        loss_sum.append(s[0])
    psnr = torch.stack(rec["psnr"])
    # the reference's compute_samples_per_subset (data/dataset_sampling.py:4-10) on a dozen (pixels, N_rand) pairs, unequal
    # sizes among them: rows (pixels, N_rand, samples_per_subset, normal_subsets, extra_sample_subsets)
    from data.dataset_sampling import compute_samples_per_subset
    subsets = [(n, r) + tuple(compute_samples_per_subset(n, 2 * r)) for n, r in SUBSET_CASES]
    MG.npz("g10_camera_code_opt", H=H, W=W, N_samples=NS, N_importance=NI, N_rand=N_RAND, n_cam=N_CAM, near=NEAR, far=FAR,
           intrinsic=intrinsic, pose=pose, view_weight_extra_coarse=extras[0], view_weight_extra_fine=extras[1],
           cam_target=torch.tensor(CAM_TARGET), image=image, rgb_at_zero=rgb_zero, n_batches=per,
           cam=torch.stack(rec["cam"]), grad=torch.stack(rec["grad"]), lr=torch.tensor(rec["lr"], dtype=torch.float64),
           loss_sum=torch.stack(loss_sum), psnr=psnr, best_cam=kw["embedded_cam"].detach(), best_psnr=psnr.max(),
           best_iter=int(torch.argmax(psnr)), subset_cases=torch.tensor(subsets, dtype=torch.int64))


if __name__ == "__main__":
    main()
