"""fp64 restatement of the held-out view metrics (test infrastructure only): skimage 0.19.3's
structural_similarity(clamp(pred, 0, 1), target, data_range=1, channel_axis=-1) with its defaults (7x7 box windows,
sample covariance, K1 = 0.01, K2 = 0.03, the mean over the window-complete interior, then over the channels), the
sums of squares behind img2mse, and compute_rmse's sums over a depth mask."""
import numpy as np

WIN = 7
C1, C2 = 0.01 ** 2, 0.03 ** 2
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)


def _window_means(a):
    """Means of every whole 7x7 window of a [H,W] fp64 plane: [H-6, W-6] (output pixel (r, c) = window centre
    (r + 3, c + 3)), horizontal 7-sums first, then vertical."""
    H, W = a.shape
    rows = sum(a[:, k:W - WIN + 1 + k] for k in range(WIN))
    return sum(rows[k:H - WIN + 1 + k, :] for k in range(WIN)) / (WIN * WIN)


def ssim_channel(x, y):
    """Mean S of one channel over [3, H-3) x [3, W-3); x, y [H,W] fp64."""
    ux, uy = _window_means(x), _window_means(y)
    uxx, uyy, uxy = _window_means(x * x), _window_means(y * y), _window_means(x * y)
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.mean()


def ssim(pred, target):
    """pred, target [H,W,3] (any float type; pred is clamped to [0, 1] first, NaN kept)."""
    x = np.clip(np.asarray(pred, dtype=np.float64), 0.0, 1.0)
    y = np.asarray(target, dtype=np.float64)
    if x.shape[0] < WIN or x.shape[1] < WIN:
        raise ValueError("smaller than one 7x7 window")
    return float(np.mean([ssim_channel(x[..., c], y[..., c]) for c in range(x.shape[-1])]))


def sse(pred, target):
    d = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    return float((d * d).sum())


def depth_sums(depth, target_depth, valid):
    """(sum of squared differences, count) over the pixels where valid is set."""
    m = np.asarray(valid).astype(bool)
    d = np.asarray(depth, dtype=np.float64)[m] - np.asarray(target_depth, dtype=np.float64)[m]
    return float((d * d).sum()), int(m.sum())
