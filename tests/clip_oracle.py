"""Float64 numpy restatement of global-norm gradient clipping as the optimiser phase applies it (mbx_grad_sqnorm,
mbx_clip_finalize, mbx_rmsprop_ema_step_clipped): the clipped vector is the one the optimiser consumes, g' = g + wd * w per
range (g' = g where wd = 0) -- what tf.clip_by_global_norm would see on the reference's total_loss, which contains slim's
regulariser.  A plain module (no test in it), like focal_oracle.py."""
import numpy as np


def opt_grad(g, w=None, wd=0.0):
    """g' of one range in float64 from float32 inputs (wd is the float32 value the kernel is handed)."""
    g = np.asarray(g, np.float64)
    return g if not wd else g + np.float64(np.float32(wd)) * np.asarray(w, np.float64)


def global_norm(ranges):
    """sqrt(sum g'^2) over `ranges`: an iterable of (g, w_or_None, wd)."""
    return float(np.sqrt(sum(float(np.sum(opt_grad(g, w, wd) ** 2)) for g, w, wd in ranges)))


def clip_scale(norm, max_norm):
    """max_norm / norm when the norm is over max_norm, else 1 (also for a norm of 0 and for max_norm = inf)."""
    return float(max_norm) / norm if norm > max_norm else 1.0


def clip(ranges, max_norm):
    """(norm, scale, [scale * g' per range]) in float64."""
    ranges = list(ranges)
    norm = global_norm(ranges)
    scale = clip_scale(norm, max_norm)
    return norm, scale, [scale * opt_grad(g, w, wd) for g, w, wd in ranges]


def clip_block(ranges, max_norm, ctl=(0.0, 0.0)):
    """The eight float32 words mbx_clip_finalize writes (include/mbx.h)."""
    with np.errstate(over="ignore", invalid="ignore"):
        total = sum(float(np.sum(opt_grad(g, w, wd) ** 2)) for g, w, wd in ranges)
        finite = bool(np.isfinite(total))
        norm = float(np.sqrt(total))
    clipped = finite and norm > max_norm
    scale = float(max_norm) / norm if clipped else 1.0
    return np.array([ctl[0], ctl[1] + (0.0 if finite else 1.0), scale, norm, float(clipped), 0, 0, 0], np.float32)
