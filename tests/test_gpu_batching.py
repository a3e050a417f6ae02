"""The use_batching ray source on a real MI355X (train.RayBank, plnerf_select_bank_rays, TrainStep.step_batch): the
bank's rays against get_rays and plnerf_select_rays bit for bit, one epoch as a permutation of the bank with its short
last batch, step_batch against TrainStep.__call__ on the same columns, resuming mid-epoch, and the data-parallel split of
a global batch whose tail is shorter than the world (a rank with no rays)."""
import os
import subprocess
import sys

import pytest
import torch

from abi_support import ROOT
from gpu_support import P, g, nvs_nets, scene
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu


def test_bank_rays_are_get_rays_of_the_training_views(P):
    H, W, i_train = 12, 17, [4, 1, 3]
    poses, images, K = scene(P, 5, H, W)
    bank = P.RayBank(images, poses, K, i_train, 2.0, 6.0, seed=7)
    assert bank.M == 3 * H * W
    cols, target, idx = bank.select(0, 0, bank.M, want_index=True)
    t, row, col = (x.cpu() for x in P.RayBank.decode(idx, H, W))
    assert sorted(idx.cpu().tolist()) == list(range(bank.M))             # one epoch: every pixel of every training view
    view = torch.tensor(i_train)[t]
    assert set(view.tolist()) == set(i_train)                           # only (and all of) the training views appear
    o, d, vd = cols.rays_o.cpu(), cols.rays_d.cpu(), cols.viewdirs.cpu()
    for v in range(5):
        m = view == v
        if v not in i_train:
            assert not m.any()
            continue
        o_ref, d_ref = orc.get_rays(H, W, K, poses[v][:3, :4])
        assert torch.equal(o[m], o_ref[row[m], col[m]]) and torch.equal(d[m], d_ref[row[m], col[m]]), v
        # every pixel of the view through plnerf_select_rays: the same direction and view direction bits
        sc, _, pix = P.select_view_rays(H, W, K, poses[v][:3, :4], None, H * W, 2.0, 6.0, seed=1, step=0, want_pixels=True)
        vd_map = torch.empty(H, W, 3)
        d_map = torch.empty(H, W, 3)
        pix = pix.long().cpu()
        vd_map[pix[:, 0], pix[:, 1]] = sc.viewdirs.cpu()
        d_map[pix[:, 0], pix[:, 1]] = sc.rays_d.cpu()
        assert torch.equal(vd[m], vd_map[row[m], col[m]]) and torch.equal(d[m], d_map[row[m], col[m]]), v
    assert torch.equal(target.cpu(), images[view, row, col])
    assert (cols.near == 2.0).all() and (cols.far == 6.0).all()
    # a slice of the epoch is that slice of the order, with every column; no view directions when not wanted
    c2, t2, i2 = bank.select(0, 100, 50, want_index=True)
    assert torch.equal(i2, idx[100:150]) and torch.equal(t2, target[100:150]) and torch.equal(c2.rays_d, cols.rays_d[100:150])
    assert torch.equal(c2.viewdirs, cols.viewdirs[100:150]) and torch.equal(c2.rays_o, cols.rays_o[100:150])
    assert bank.select(0, 100, 50, want_viewdirs=False)[0].viewdirs is None
    # the seed keys the order
    other = P.RayBank(images, poses, K, i_train, 2.0, 6.0, seed=8).select(0, 0, bank.M, want_index=True)[2]
    assert not torch.equal(other, idx)


def test_one_epoch_is_a_permutation_with_a_short_tail(P):
    H, W = 12, 17
    poses, images, K = scene(P, 3, H, W)
    bank = P.RayBank(g(images), poses, K, [0, 1, 2], 0.0, 1.0, seed=2)
    M, n_rand = 612, 50
    assert bank.M == M
    epochs = []
    for e in range(2):
        parts = []
        for k in range(13):
            cols, target, idx, off, n = bank.batch(13 * e + k, n_rand, want_index=True)
            assert off == 0 and n == idx.numel() == cols.shape[0] == target.shape[0] == (12 if k == 12 else 50)
            parts.append(idx.cpu())
        order = torch.cat(parts)
        assert sorted(order.tolist()) == list(range(M))
        epochs.append(order)
    assert not torch.equal(epochs[0], epochs[1])
    assert bank.schedule(26, n_rand) == (2, 0, 50)
    with pytest.raises(RuntimeError, match=r"code -3"):      # PLNERF_ERANGE: positions past the epoch's end
        bank.select(0, 600, 13)
    with pytest.raises(RuntimeError, match=r"code -3"):
        bank.select(0, M, 1)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("dataset", ["llff", "blender"])
def test_step_batch_equals_call_on_the_same_columns(P, precision, dataset):
    """step_batch is the loop body on the bank's batch: bit-identical to TrainStep.__call__ given the same RayColumns
    and targets, three steps through the short last batch of epoch 0 into epoch 1.  llff: NDC rays, near 0 / far 1,
    raw_noise_std 1, no white background; blender: white background, near 2 / far 6."""
    H, W = 10, 13
    llff = dataset == "llff"
    over = dict(dataset=dataset, white_bkgd=not llff, raw_noise_std=1.0 if llff else 0.0)
    poses, images, K = scene(P, 5, H, W, forward_facing=llff, seed=3)
    near, far = (0.0, 1.0) if llff else (2.0, 6.0)
    bank = P.RayBank(images, poses, K, [0, 2, 3], near, far, seed=5)
    n_rand, start = 128, 2                   # M = 390: steps 2, 3, 4 take 128, 6 and (epoch 1) 128 rays
    args, kw, opt, opt_c = nvs_nets(P, precision, **over)
    assert bool(kw.get("ndc", True)) == llff
    ts = P.TrainStep(args, kw, opt, opt_c, start=start, distributed=False, seed=5)
    args2, kw2, opt2, opt_c2 = nvs_nets(P, precision, **over)
    ts2 = P.TrainStep(args2, kw2, opt2, opt_c2, start=start, distributed=False, seed=5)
    sizes = []
    for step in range(start, start + 3):
        cols, target, _, off, n = bank.batch(step, n_rand)
        loss2, psnr2 = ts2(H, W, bank.K, cols, target, near=near, far=far)
        loss, psnr = ts.step_batch(bank, n_rand)
        sizes.append(ts.last_batch[2])
        assert torch.equal(loss, loss2) and torch.equal(psnr, psnr2), (step, float(loss), float(loss2))
        assert torch.isfinite(loss)
    assert sizes == [128, 6, 128]
    for a, b in zip(ts.nets, ts2.nets):
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)
    with pytest.raises(ValueError):
        ts.step_batch(bank, n_rand, precrop=(2, 2))


def test_resume_continues_the_same_order(P):
    H, W = 10, 13
    poses, images, K = scene(P, 5, H, W)
    bank = P.RayBank(images, poses, K, [1, 2, 4], 2.0, 6.0, seed=9)
    n_rand, s = 128, 5                       # M = 390, 4 steps per epoch: step 5 is position 128 of epoch 1
    args, kw, opt, opt_c = nvs_nets(P)
    ts = P.TrainStep(args, kw, opt, opt_c, distributed=False, seed=9)
    for _ in range(s + 1):
        ts.step_batch(bank, n_rand)
    from_zero = ts.last_batch
    args2, kw2, opt2, opt_c2 = nvs_nets(P)
    ts2 = P.TrainStep(args2, kw2, opt2, opt_c2, start=s, distributed=False, seed=9)
    ts2.step_batch(bank, n_rand)
    assert ts2.last_batch == from_zero == (1, 128, 128, 0, 128)
    idx_a = bank.select(from_zero[0], from_zero[1], from_zero[2], want_index=True)[2]
    idx_b = bank.batch(s, n_rand, want_index=True)[2]
    assert torch.equal(idx_a, idx_b)


_DP_BATCH_WORKER = r"""
import hashlib, os, sys, tempfile, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import plnerf_amd as P
from plnerf_amd import dp
from oracle import plnerf_oracle as orc
from run_args import nvs_args
VIEWS = [int(v) for v in sys.argv[2].split(",")]
H, W, N_RAND, START, STEPS = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), 3
BOUND = float(sys.argv[7])
rank, world, _ = dp.init_from_env(backend="gloo")          # every rank on cuda:0; gloo moves CUDA tensors through the host
dev = torch.device("cuda:0")
torch.cuda.set_device(0)


def make(distributed):
    d = tempfile.mkdtemp(); os.makedirs(os.path.join(d, "exp"))
    args = nvs_args(d, "f16x3", N_rand=256)
    kw, _, _, _, opt, opt_c = P.create_nerf(args, device=dev)
    kw["network_fn"].load_state_dict(orc.closed_form_state_dict(0, False))
    kw["network_fine"].load_state_dict(orc.closed_form_state_dict(1, False))
    return kw, P.TrainStep(args, kw, opt, opt_c, start=START, distributed=distributed, seed=3)


poses = torch.stack([P.rays.pose_spherical(-180.0 + 72.0 * i, -30.0, 4.0) for i in range(5)])
yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
images = torch.stack([torch.stack([xx, yy, 0.5 * (xx + yy)], -1).roll(3 * i, 1) for i in range(5)])
K = [[1.4 * W, 0, W / 2], [0, 1.4 * W, H / 2], [0, 0, 1]]
bank = P.RayBank(images, poses, K, VIEWS, 2.0, 6.0, seed=3)
kw, ts = make(True)
assert ts.bucket is not None and ts.world == world
n_params = [sum(p.numel() for p in n.parameters()) for n in ts.nets]
TAIL = dp.GradientBucket.TAIL
seen = []
_all_reduce = dist.all_reduce


def spy(t, *a, **k):          # this rank's contribution to each gradient exchange, as it enters the collective
    if torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32:
        seen.append(t.detach().clone())
    return _all_reduce(t, *a, **k)


dist.all_reduce = spy


def grad_absmax(buf):
    if buf.numel() == sum(n_params) + TAIL * len(n_params):     # both networks back to back, each with its status tail
        parts, off = [], 0
        for k in n_params:
            parts.append(buf[off:off + k])
            off += k + TAIL
    else:
        assert buf.numel() in [k + TAIL for k in n_params], buf.numel()
        parts = [buf[:-TAIL]]
    return max(float(p.abs().max()) for p in parts)


zero_steps, tail_steps = 0, 0
for k in range(STEPS):
    seen.clear()
    gs = ts.global_step
    epoch, p0, n = bank.schedule(gs, N_RAND * world)
    b, e = dp.shard_batch(n, rank, world)
    loss, psnr = ts.step_batch(bank, N_RAND)
    assert ts.last_batch == (epoch, p0 + b, e - b, b, n), (ts.last_batch, (epoch, p0 + b, e - b, b, n))
    assert ts.bucket.pending() == 0 and ts.bucket.collectives == 1 and len(seen) == 1, (ts.bucket.collectives, len(seen))
    gmax = grad_absmax(seen[0])
    tail_steps += n < N_RAND * world
    if e == b:
        zero_steps += 1
        assert gmax == 0.0, f"rank {rank}: a rank without rays contributed {gmax}"
        assert torch.isnan(loss) and torch.isnan(psnr)
    else:
        assert gmax > 0.0 and torch.isfinite(loss), (gmax, float(loss))
dist.all_reduce = _all_reduce
assert tail_steps == 1, "the steps must cross the epoch boundary through the short batch"
counts = [None] * world
dist.all_gather_object(counts, zero_steps)
assert sum(counts) >= 1, "no rank was left without rays"
flat = torch.cat([p.detach().reshape(-1) for n in ts.nets for p in n.parameters()]).cpu()
digest = hashlib.sha256(flat.numpy().tobytes()).hexdigest()
gathered = [None] * world
dist.all_gather_object(gathered, digest)
assert all(gd == gathered[0] for gd in gathered), "replicas diverged"
if rank == 0:
    # the same steps as ONE process over the global batch (same bank order, same draws)
    kw1, ts1 = make(False)
    for step in range(STEPS):
        ts1.step_batch(bank, world * N_RAND)
    worst = max(float((p.detach() - q.detach()).abs().max()) for n, m in zip(ts.nets, ts1.nets)
                for p, q in zip(n.parameters(), m.parameters()))
    print(f"max |param({world} ranks) - param(1 rank)| =", worst, "zero-ray steps per rank", counts)
    assert worst <= BOUND, (worst, BOUND)
print(f"rank {rank} ok")
dist.destroy_process_group()
"""


# bound: the 2e-4 of test_gpu_step.py's data-parallel tests for two ranks.  Three ranks land at 2.4e-4 - 2.8e-4 (measured
# at 128 and 1024 rays per rank): 1 / 3 is not exact in fp32, unlike the 1 / 2 and 1 / 4 of the existing tests, and three
# Adam steps amplify the rounding of small gradients -- bounded here at 3e-4.
@pytest.mark.parametrize("world,views,H,W,n_rand,start,bound", [
    (2, "4,0,2", 9, 19, 128, 1, 2e-4),      # M = 513, B = 256: steps 1, 2, 3 take 256, 1 (rank 1: none), epoch 1's first 256
    (3, "3,1", 29, 53, 1024, 0, 3e-4),      # M = 3074, B = 3072: steps 0, 1, 2 take 3072, 2 (rank 2: none), epoch 1's first 3072
])
def test_data_parallel_batches_across_a_short_tail(P, tmp_path, world, views, H, W, n_rand, start, bound):
    """Gloo ranks on one GPU (the pattern of test_gpu_step.py's data-parallel tests) step the bank through an epoch
    boundary whose last batch is shorter than the world: replicas stay bit-identical, the rank without rays sends an
    exactly zero gradient into the same single collective, and the weights land within `bound` of one process stepping
    the whole global batch."""
    script = tmp_path / "dp_batch_worker.py"
    script.write_text(_DP_BATCH_WORKER)
    port = 30300 + (os.getpid() % 200) + 200 * (world > 2)
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT, views, str(H), str(W), str(n_rand), str(start),
                                       str(bound)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=600)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {rank} failed:\n{out[-3000:]}"
        assert f"rank {rank} ok" in out
    print([l for l in outs[0].splitlines() if l.startswith("max |param")])
