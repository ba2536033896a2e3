"""numpy float64 restatement of mbx_match_tal (include/mbx.h): task-aligned matching behind the bipartite match.  Plain loops
per image and box; every float64 operation is the header's, in its order, so `match`, `n_extra` and `thr` are compared bit
for bit with the kernel's."""
import numpy as np

from tests.atss_oracle import centres


def alpha_halves(alpha):
    """alpha as the number of halves the C ABI takes; alpha must be a multiple of 0.5."""
    h = int(round(float(alpha) * 2))
    assert h / 2.0 == float(alpha), alpha
    return h


def overlaps(decoded, box):
    """u float64 [P]: the IoU of every decoded prediction [P,4] with the box, the prediction first, the corners as they are:
    iw = min(x2) - max(x1), ih likewise; inter = iw > 0 and ih > 0 ? iw * ih : 0; uni = area_e + area_j - inter;
    u = uni > 0 ? inter / uni : 0.  (min / max as fmin / fmax: a NaN operand gives the other one.)"""
    e = np.asarray(decoded, np.float32).astype(np.float64).reshape(-1, 4)
    g = np.asarray(box, np.float32).astype(np.float64).reshape(4)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        area_e = (e[:, 2] - e[:, 0]) * (e[:, 3] - e[:, 1])
        area_g = (g[2] - g[0]) * (g[3] - g[1])
        iw = np.fmin(e[:, 2], g[2]) - np.fmax(e[:, 0], g[0])
        ih = np.fmin(e[:, 3], g[3]) - np.fmax(e[:, 1], g[1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
        uni = area_e + area_g - inter
        return np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)


def metric(conf, u, halves, beta):
    """t float64 [P] = s^(halves / 2) * u^beta by repeated products: r = 1; halves // 2 times r = r * s; an odd half:
    r = r * sqrt(s); w = 1; beta times w = w * u; t = r * w."""
    s = np.asarray(conf, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        r = np.ones_like(s)
        for _ in range(halves // 2):
            r = r * s
        if halves % 2:
            r = r * np.sqrt(s)
        w = np.ones_like(u)
        for _ in range(beta):
            w = w * u
        return r * w


def inside(priors, box):
    """bool [P]: the prior's own centre lies strictly inside the box."""
    cx, cy = centres(priors)
    g = np.asarray(box, np.float32).astype(np.float64).reshape(4)
    with np.errstate(invalid="ignore"):
        return (g[0] < cx) & (cx < g[2]) & (g[1] < cy) & (cy < g[3])


def select(priors, decoded, conf, box, topk, halves, beta):
    """(selected priors in rank order, u [P], t [P], candidate mask [P]) of one box: the min(topk, candidates) largest t,
    equal t to the lowest index -- picked one at a time."""
    u = overlaps(decoded, box)
    t = metric(conf, u, halves, beta)
    with np.errstate(invalid="ignore"):
        cand = inside(priors, box) & (t > 0)
    left = [int(p) for p in np.nonzero(cand)[0]]
    picked = []
    while left and len(picked) < int(topk):
        best = left[0]
        for p in left[1:]:                                     # ascending index: a strictly larger t only
            if t[p] > t[best]:
                best = p
        picked.append(best)
        left.remove(best)
    return picked, u, t, cand


def tal(priors, decoded, conf, gt, n_gt, status, match, topk, alpha=1.0, beta=6):
    """(match int32 [B,P], n_extra int32 [B], thr float64 [B,G])."""
    priors, gt = np.asarray(priors, np.float32), np.asarray(gt, np.float32)
    decoded, conf = np.asarray(decoded, np.float32), np.asarray(conf, np.float32)
    halves, beta = alpha_halves(alpha), int(beta)
    assert 0 <= halves <= 8 and 1 <= beta <= 16 and int(topk) >= 1
    out = np.array(match, np.int32, copy=True)
    B, P = out.shape
    G = gt.shape[1]
    n_extra = np.zeros(B, np.int32)
    thr = np.zeros((B, G), np.float64)
    for b in range(B):
        n = int(n_gt[b])
        if int(status[b]) != 0 or n <= 0 or n > G:
            continue
        best_u, best_j = {}, {}
        for j in range(n):
            picked, u, t, _ = select(priors, decoded[b], conf[b], gt[b, j], topk, halves, beta)
            if picked:
                thr[b, j] = t[picked[-1]]
            for p in picked:
                if out[b, p] < 0 and (p not in best_u or u[p] > best_u[p]):     # strictly larger: the lowest j stays
                    best_u[p], best_j[p] = u[p], j
        for p, j in best_j.items():
            out[b, p] = j
        n_extra[b] = len(best_j)
    return out, n_extra, thr


def tal_sorted(priors, decoded, conf, gt, n_gt, status, match, topk, alpha=1.0, beta=6):
    """The same result by another route (test_tal_cpu.py compares the two): per box one lexsort by (-t, index), then per
    prior an argmax over the boxes that selected it."""
    priors, gt = np.asarray(priors, np.float32), np.asarray(gt, np.float32)
    decoded, conf = np.asarray(decoded, np.float32), np.asarray(conf, np.float32)
    halves, beta = alpha_halves(alpha), int(beta)
    out = np.array(match, np.int32, copy=True)
    B, P = out.shape
    G = gt.shape[1]
    n_extra = np.zeros(B, np.int32)
    thr = np.zeros((B, G), np.float64)
    for b in range(B):
        n = int(n_gt[b])
        if int(status[b]) != 0 or n <= 0 or n > G:
            continue
        chosen = np.zeros((n, P), bool)
        us = np.zeros((n, P), np.float64)
        for j in range(n):
            us[j] = overlaps(decoded[b], gt[b, j])
            t = metric(conf[b], us[j], halves, beta)
            with np.errstate(invalid="ignore"):
                idx = np.nonzero(inside(priors, gt[b, j]) & (t > 0))[0]
            order = idx[np.lexsort((idx, -t[idx]))][:int(topk)]
            chosen[j, order] = True
            if len(order):
                thr[b, j] = t[order[-1]]
        free = (out[b] < 0) & chosen.any(0)
        for p in np.nonzero(free)[0]:
            out[b, p] = int(np.argmax(np.where(chosen[:, p], us[:, p], -1.0)))     # the first of equal maxima
        n_extra[b] = int(free.sum())
    return out, n_extra, thr
