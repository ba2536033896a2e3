"""numpy restatement of mbx_loss_fwd_bwd_mined (include/mbx.h): which negatives hard-negative mining keeps, and the loss
and gradients that follow.  The selection is integer work on float bits, so it is exact; the values come from the float64
formulas of oracle.ref_numpy.add_loss / add_loss_grads, fed the selection."""
import numpy as np

from oracle import ref_numpy as R


def score_order_key(x):
    """uint32 image of float32 bits that orders like the floats (csrc/boxes.h: score_order_key): -0 == +0, a NaN on top."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key = np.where(x == 0, np.uint32(0x80000000), key)
    return np.where(np.isnan(x), np.uint32(0xffffffff), key).astype(np.uint32)


def mining_order(conf_in_row, match_row):
    """The negatives of one image, best first: key descending, bit-equal keys by ascending index (a stable sort)."""
    neg = np.nonzero(np.asarray(match_row) < 0)[0]
    key = score_order_key(np.asarray(conf_in_row, np.float32)[neg]).astype(np.int64)
    return neg[np.argsort(-key, kind="stable")]


def n_selected(match, neg_per_pos, min_neg):
    """K per image: min(N_neg, max(min_neg, neg_per_pos * n_pos)) in Python integers."""
    match = np.asarray(match)
    P = match.shape[1]
    out = []
    for m in match:
        n_pos = int((m >= 0).sum())
        out.append(min(P - n_pos, max(int(min_neg), int(neg_per_pos) * n_pos)))
    return np.array(out, np.int32)


def select(conf_in, match, neg_per_pos, min_neg):
    """(mask bool [B,P] of the selected negatives, n_neg int32 [B])."""
    conf_in, match = np.asarray(conf_in, np.float32), np.asarray(match)
    K = n_selected(match, neg_per_pos, min_neg)
    mask = np.zeros(match.shape, bool)
    for b in range(match.shape[0]):
        mask[b, mining_order(conf_in[b], match[b])[:K[b]]] = True
    return mask, K


def mined_loss(decoded, conf_in, conf_is_logit, gt, match, alpha, neg_per_pos, min_neg):
    """dict(mask, n_neg, loc_loss, conf_loss, d_locs, d_conf_in) for grad_scale = 1.  `decoded` are prior-decoded
    locations, as the C ABI takes them.  An unselected negative is given the confidence 0 (the logit -inf): ref_numpy's
    negative term is then -log((1 - 1e-10) + 1e-10) = -log(1) = 0 in float32 and its gradient s (1 - s) / u = 0, exactly,
    so its own formulas return the mined sums."""
    decoded, conf_in = np.asarray(decoded, np.float32), np.asarray(conf_in, np.float32)
    match = np.asarray(match)
    B, P = match.shape
    mask, K = select(conf_in, match, neg_per_pos, min_neg)
    dropped = (match < 0) & ~mask
    n = (match >= 0).sum(1).astype(np.int32)
    zero_priors = np.zeros((P, 4), np.float32)
    with np.errstate(over="ignore"):
        if conf_is_logit:
            z = np.where(dropped, np.float32(-np.inf), conf_in).astype(np.float32)
            ref = R.add_loss(decoded, R.sigmoid_f32(z), gt, n, zero_priors, alpha, match=match)
            d_locs, d_in = R.add_loss_grads(decoded, z, gt, zero_priors, alpha, match)
        else:
            c_in = np.where(dropped, np.float32(0), conf_in).astype(np.float32)
            ref = R.add_loss(decoded, c_in, gt, n, zero_priors, alpha, match=match)
            # d/d confidence of ref_numpy.add_loss's terms, float64: -1/c on a positive, 1/u on a selected negative
            c = (conf_in + np.float32(R.SMALL_EPSILON)).astype(np.float32)
            u = ((np.float32(1.0) - c) + np.float32(R.SMALL_EPSILON)).astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                d_in = np.where(match >= 0, -1.0 / c.astype(np.float64), np.where(mask, 1.0 / u.astype(np.float64), 0.0))
            d_in = d_in.astype(np.float32)
            d_locs, _ = R.add_loss_grads(decoded, np.zeros((B, P), np.float32), gt, zero_priors, alpha, match)
    return dict(mask=mask, n_neg=K, loc_loss=ref["loc_loss"], conf_loss=ref["conf_loss"], d_locs=d_locs, d_conf_in=d_in)
