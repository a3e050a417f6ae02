"""fp64 restatement of the importance-sampling error (test infrastructure only): test_images_samples of
depth_supervised_exps/run_nerf_sample_based_depth.py:396-411 per ray -- the mean over the N hypotheses of
|pred_hyp - depth_map| -- then its sum and count over the valid rays; and the reference's own fp32 expression of a
view's mean, for comparison."""
import torch


def sample_error(pred_hyp, depth, valid=None):
    """(sum over the valid rays of mean_k |h_k - d|, number of valid rays) in fp64; pred_hyp [..., N], depth and valid
    [...] (valid None = every ray).  Works on any device."""
    h, d = torch.as_tensor(pred_hyp).double(), torch.as_tensor(depth).double()
    per_ray = (h - d[..., None]).abs().mean(-1)
    m = torch.ones_like(d, dtype=torch.bool) if valid is None else torch.as_tensor(valid).bool()
    return float(per_ray[m].sum()), int(m.sum())


def reference_view_mean(pred_hyp, depth_map, valid):
    """The reference's fp32 expression of one view's value (:396-405): NaN without a valid pixel."""
    repeated = depth_map.unsqueeze(-1).repeat(*([1] * depth_map.dim()), pred_hyp.shape[-1])
    dists = torch.norm(pred_hyp.unsqueeze(-1) - repeated.unsqueeze(-1), p=2, dim=-1)
    return torch.mean(torch.mean(dists, dim=-1)[valid])
