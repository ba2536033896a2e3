"""Numpy restatement of the layer-wise trust ratios (LARS on sgd, LAMB on adam / adamw) as the optimiser phase applies them
(mbx_trust_plan, mbx_trust_norms_sgd, mbx_trust_moments_adam, mbx_trust_ratios, mbx_sgd_ema_step_trust,
mbx_adam_ema_step_trust), on top of the oracles of tests/test_optimizer_cpu.py.

The contract restated.  The variables of one trainable range are a contiguous partition, bounds[0] = 0 < bounds[1] < ... in
range coordinates; variable i owns [bounds[i], bounds[i + 1]).  Per variable two norms, sums of squares in double over float32
values: ||w||, the weights before the step, and ||x||, where
  sgd          x = g' = clip scale * (g + wd_l2 * w), the vector the optimiser consumes;
  adam, adamw  x = u = m^ / (sqrt(v^) + eps) + wd_decoupled * w from the UPDATED moments.
r = coeff * ||w|| / ||x|| when the variable adapts and both norms are > 0, exactly 1 otherwise; computed in double and rounded to
float32 once.  sgd consumes r * g' (acc = momentum * acc + r * g'); adam steps by lr * (r * u).  No epsilon, no special case
for a non-finite norm.  Everything else -- the EMA from the weight before the step, reg_loss, the bf16 copy -- is the twins'.

Like the oracles it builds on, every function is plain arithmetic on the arrays it is handed: float64 arrays are the anchor of
tests/test_gpu_trust.py, float32 ones the restatement tests/test_trust_cpu.py holds against that anchor (the ratio is then the
float32 the kernel would store).
"""
import numpy as np

from tests import test_optimizer_cpu as OC

CHUNK_DTYPE = np.dtype([("lo", "<i8"), ("len", "<i4"), ("var", "<i4")])                              # mbx_trust_chunk
VAR_DTYPE = np.dtype([("first_chunk", "<i4"), ("n_chunks", "<i4"), ("adapt", "<i4"), ("pad", "<i4")])   # mbx_trust_var


def bounds_of(lengths, start=0):
    """bounds of consecutive variables of these lengths; start > 0 puts one more variable of that length in front."""
    return np.concatenate([[0], np.cumsum(([start] if start else []) + list(lengths))]).astype(np.int64)


def plan(bounds, CH):
    """The chunk plan: cuts on the grid of multiples of CH and at every bound.  Returns (chunks [(lo, len, var)],
    vars [(first_chunk, n_chunks)])."""
    chunks, vars_ = [], []
    for i in range(len(bounds) - 1):
        lo, hi, first = int(bounds[i]), int(bounds[i + 1]), len(chunks)
        while lo < hi:
            end = min(hi, (lo // CH + 1) * CH)
            chunks.append((lo, end - lo, i))
            lo = end
        vars_.append((first, len(chunks) - first))
    return chunks, vars_


def plan_images(bounds, adapt, CH):
    """The two host images mbx_trust_plan fills, as bytes."""
    chunks, vars_ = plan(bounds, CH)
    c = np.array(chunks, dtype=CHUNK_DTYPE)
    v = np.array([(f, n, int(bool(a)), 0) for (f, n), a in zip(vars_, adapt)], dtype=VAR_DTYPE)
    return c.tobytes(), v.tobytes()


def ratios(w, x, bounds, adapt, coeff):
    """r per variable, in the dtype of w (float32 arrays: the value the kernel stores; float64: unrounded)."""
    out = np.ones(len(bounds) - 1, np.float64)
    for i, a in enumerate(adapt):
        lo, hi = int(bounds[i]), int(bounds[i + 1])
        nw = float(np.sqrt(np.sum(w[lo:hi].astype(np.float64) ** 2)))
        nx = float(np.sqrt(np.sum(x[lo:hi].astype(np.float64) ** 2)))
        if a and nw > 0.0 and nx > 0.0:
            out[i] = OC.f32(coeff) * nw / nx
    return out.astype(w.dtype)


def per_element(r, bounds):
    return np.repeat(r, np.diff(bounds))


def lars_step(w, g, acc, bounds, adapt, coeff, lr, momentum=0.9, nesterov=False, wd=0.0, scale=None):
    """One LARS step; returns (w, acc, r)."""
    gp = OC.opt_grad(w, g, wd, scale)
    r = ratios(w, gp, bounds, adapt, coeff)
    w, acc = OC.sgd_step(w, per_element(r, bounds) * gp, acc, lr, momentum=momentum, nesterov=nesterov)
    return w, acc, r


def lamb_step(w, g, m, v, t, bounds, adapt, coeff, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, wd_decoupled=0.0, scale=None):
    """One LAMB step (t = 1: the first applied step); returns (w, m, v, r)."""
    _, m, v = OC.adam_step(w, g, m, v, t, lr, beta1, beta2, eps, wd, wd_decoupled, scale)        # the moments are Adam's
    b1, b2 = OC.f32(beta1), OC.f32(beta2)
    u = (m / (1.0 - b1 ** t)) / ((v / (1.0 - b2 ** t)) ** 0.5 + OC.f32(eps))
    if wd_decoupled:
        u = u + OC.f32(wd_decoupled) * w
    u = u.astype(w.dtype)
    r = ratios(w, u, bounds, adapt, coeff)
    return (w - OC.f32(lr) * (per_element(r, bounds) * u)).astype(w.dtype), m, v, r


# ---------------------------------------------------------------------------------------------- the data of the kernel tests
# SMALL: variables of 1, 3, 4, 5, 259, CH, CH + 1 and 2 CH + 7 in that order (bounds on odd offsets, a variable that is one
# whole chunk, one that spills by one element, one that spans grid cuts), a variable whose w is all zero, one whose g is all
# zero, two that do not adapt (8 and 3 elements).
ZERO_W, ZERO_G = 8, 9                                          # the indices of those two variables in SMALL
COEFF = 0.5                                                    # ratios of order 1: the steps are visible at the bar
SMALL_SEED = 500


def small(CH):
    """(bounds, adapt) of SMALL."""
    lengths = [1, 3, 4, 5, 259, CH, CH + 1, 2 * CH + 7, 37, 41, 8, 3]
    return bounds_of(lengths), [1] * 10 + [0, 0]


def small_data(CH, seed=SMALL_SEED):
    """(w, g, ema) float32 over SMALL: test_optimizer_cpu.kernel_data (|g| >= 0.5, so g' never cancels) with the two zeroed
    variables.  The zero-g variable has g' = wd * w: no element of it is anywhere near Adam's eps."""
    bounds, _ = small(CH)
    w, g, ema = OC.kernel_data(int(bounds[-1]), seed)
    w[bounds[ZERO_W]:bounds[ZERO_W + 1]] = 0.0
    g[bounds[ZERO_G]:bounds[ZERO_G + 1]] = 0.0
    assert np.abs(w[bounds[ZERO_G]:bounds[ZERO_G + 1]]).min() * OC.KERNEL_WD > 1e-4
    return w, g, ema


LARS_CASES = [dict(momentum=0.0, nesterov=False), dict(momentum=0.9, nesterov=False), dict(momentum=0.0, nesterov=True),
              dict(momentum=0.9, nesterov=True)]
LAMB_CASES = [dict(wd_decoupled=0.0), dict(wd_decoupled=0.01)]
CASES = [("sgd", kw) for kw in LARS_CASES] + [("adam", kw) for kw in LAMB_CASES]


def two_steps(dtype, w, g, ema, bounds, adapt, rule, kw, coeff=COEFF, wd=OC.KERNEL_WD, scale=None):
    """Two steps of LARS / LAMB from zero slots in `dtype`: [(w, slot a, slot b, ema, r)] after each."""
    w, g, ema = (np.asarray(x, dtype) for x in (w, g, ema))
    a, b = np.zeros_like(w), np.zeros_like(w)
    out = []
    for k in (1, 2):
        ema = OC.ema_step(ema, w, OC.KERNEL_HYPER["d"])
        if rule == "sgd":
            w, a, r = lars_step(w, g, a, bounds, adapt, coeff, OC.KERNEL_HYPER["lr"], wd=wd, scale=scale, **kw)
        else:
            w, a, b, r = lamb_step(w, g, a, b, k, bounds, adapt, coeff, OC.KERNEL_HYPER["lr"], wd=wd, scale=scale, **kw)
        out.append((w, a, b, ema, r))
    return out
