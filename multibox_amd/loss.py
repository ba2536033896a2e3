"""Matching + loss -- host mirror of the reference's loss.py on libmbx.

``compute_assignments`` and ``add_loss`` keep the reference's names and argument meaning
(loss.py:8, loss.py:55); tensors are torch CUDA tensors instead of TF tensors.
``MultiboxLoss`` is the fused training entry (decode -> match -> loss + gradients), all
on the caller's stream, graph-capturable.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .config import LOC_LOSS_TYPES as LOC_TYPES

SMALL_EPSILON = 1e-10   # loss.py:6


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "expected contiguous float32 CUDA tensor"
    return t


def _i32(t):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), "expected contiguous int32 CUDA tensor"
    return t


def match_boxes(decoded, conf, gt_bboxes, num_gt_bboxes, alpha, match=None, status=None):
    """mbx_match: decoded [B,P,4], conf [B,P] (+1e-10 applied), gt [B,G,4], n [B] -> match int32 [B,P]."""
    B, P = decoded.shape[0], decoded.shape[1]
    G = gt_bboxes.shape[1]
    if match is None:
        match = torch.empty((B, P), dtype=torch.int32, device=decoded.device)
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=decoded.device)
    _lib.check(_lib.lib().mbx_match(_f32(decoded).data_ptr(), _f32(conf).data_ptr(), _f32(gt_bboxes).data_ptr(),
                                    _i32(num_gt_bboxes).data_ptr(), float(alpha), B, P, G, match.data_ptr(),
                                    status.data_ptr(), None, 0, _stream()), "mbx_match")
    return match, status


def extend_matches(priors, gt_bboxes, num_gt_bboxes, status, match, iou_threshold, n_extra=None):
    """mbx_match_extend (threshold matching, SSD section 2.2): priors [P,4] corners, gt [B,G,4], n [B], status [B] as
    mbx_match left it, match int32 [B,P] updated IN PLACE -- every prior still unmatched goes to the box it overlaps
    most if that IoU is over iou_threshold, in (0, 1].  n_extra int32 [B] (optional) receives the number added per image.
    Returns (match, n_extra)."""
    B, P = match.shape
    G = gt_bboxes.shape[1]
    assert priors.shape == (P, 4) and gt_bboxes.shape == (B, G, 4)
    _lib.check(_lib.lib().mbx_match_extend(_f32(priors).data_ptr(), _f32(gt_bboxes).data_ptr(),
                                           _i32(num_gt_bboxes).data_ptr(), _i32(status).data_ptr(), float(iou_threshold),
                                           B, P, G, _i32(match).data_ptr(),
                                           None if n_extra is None else _i32(n_extra).data_ptr(), _stream()),
               "mbx_match_extend")
    return match, n_extra


def ignore_matches(boxes, gt_bboxes, num_gt_bboxes, status, match, iou_threshold, n_ignored=None):
    """mbx_match_ignore (the ignore band behind the matching): boxes [P,4] corners -- the priors, shared by all images -- or
    [B,P,4], a row per image (the decoded predictions), gt [B,G,4], n [B], status [B] as mbx_match left it, match int32
    [B,P] updated IN PLACE -- every prior still free (-1) that overlaps some box of its image by at least iou_threshold, in
    (0, 1], becomes -2 (MBX_MATCH_IGNORED), which mbx_loss_fwd_bwd_ignore leaves out of the confidence loss.  n_ignored
    int32 [B] (optional) receives the number ignored per image.  Returns (match, n_ignored)."""
    B, P = match.shape
    G = gt_bboxes.shape[1]
    assert boxes.shape in ((P, 4), (B, P, 4)) and gt_bboxes.shape == (B, G, 4)
    _lib.check(_lib.lib().mbx_match_ignore(_f32(boxes).data_ptr(), int(boxes.dim() == 3), _f32(gt_bboxes).data_ptr(),
                                           _i32(num_gt_bboxes).data_ptr(), _i32(status).data_ptr(), float(iou_threshold),
                                           B, P, G, _i32(match).data_ptr(),
                                           None if n_ignored is None else _i32(n_ignored).data_ptr(), _stream()),
               "mbx_match_ignore")
    return match, n_ignored


def _level_table(level_start):
    """level_start as the int32 HOST array mbx_match_atss takes, and its number of levels."""
    levels = [int(v) for v in level_start]
    return (ctypes.c_int32 * len(levels))(*levels), len(levels) - 1


def atss_matches(priors, level_start, gt_bboxes, num_gt_bboxes, status, match, topk, n_extra=None, thr=None):
    """mbx_match_atss (ATSS matching, Zhang et al. 2020): priors [P,4] corners, level_start the HOST list [0, ..., P] of
    the pyramid levels, gt [B,G,4], n [B], status [B] as mbx_match left it, match int32 [B,P] updated IN PLACE -- per box
    the topk priors nearest to its centre on every level are candidates, its threshold is the mean plus the standard
    deviation of their IoUs, and every free prior that is a candidate at or over it with its centre inside the box goes to
    the box of the largest IoU.  n_extra int32 [B] and thr float64 [B,G] (both optional) receive the number added per
    image and the thresholds.  Returns (match, n_extra, thr)."""
    B, P = match.shape
    G = gt_bboxes.shape[1]
    assert priors.shape == (P, 4) and gt_bboxes.shape == (B, G, 4)
    assert thr is None or (thr.is_cuda and thr.dtype == torch.float64 and thr.is_contiguous() and thr.shape == (B, G))
    table, n_levels = _level_table(level_start)
    _lib.check(_lib.lib().mbx_match_atss(_f32(priors).data_ptr(), table, n_levels, _f32(gt_bboxes).data_ptr(),
                                         _i32(num_gt_bboxes).data_ptr(), _i32(status).data_ptr(), int(topk), B, P, G,
                                         _i32(match).data_ptr(), None if n_extra is None else _i32(n_extra).data_ptr(),
                                         None if thr is None else thr.data_ptr(), _stream()), "mbx_match_atss")
    return match, n_extra, thr


TAL_ALPHA_DEFAULT, TAL_BETA_DEFAULT = 1.0, 6                  # TOOD's setting


def _tal_arguments(tal_topk, tal_alpha, tal_beta):
    """None (off), or (topk, alpha_halves, beta) as mbx_match_tal takes them.  Raises ValueError on a bad value."""
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if tal_topk is None:
        if tal_alpha != TAL_ALPHA_DEFAULT or tal_beta != TAL_BETA_DEFAULT or isinstance(tal_alpha, bool) \
                or isinstance(tal_beta, bool):
            raise ValueError("tal_alpha / tal_beta are given without tal_topk")
        return None
    if not (isinstance(tal_topk, int) and not isinstance(tal_topk, bool) and 1 <= tal_topk <= 2 ** 31 - 1):
        raise ValueError("tal_topk must be an int >= 1, got %r" % (tal_topk,))
    if not (number(tal_alpha) and 0.0 <= tal_alpha <= 4.0 and tal_alpha * 2 == int(tal_alpha * 2)):
        raise ValueError("tal_alpha must be a multiple of 0.5 in [0, 4], got %r" % (tal_alpha,))
    if not (number(tal_beta) and 1 <= tal_beta <= 16 and tal_beta == int(tal_beta)):
        raise ValueError("tal_beta must be an int in [1, 16], got %r" % (tal_beta,))
    return tal_topk, int(tal_alpha * 2), int(tal_beta)


def tal_matches(priors, decoded, conf, gt_bboxes, num_gt_bboxes, status, match, topk, alpha=TAL_ALPHA_DEFAULT,
                beta=TAL_BETA_DEFAULT, n_extra=None, thr=None):
    """mbx_match_tal (task-aligned matching, TOOD, Feng et al. 2021): priors [P,4] corners, decoded [B,P,4] and conf [B,P]
    as mbx_match reads them, gt [B,G,4], n [B], status [B] as mbx_match left it, match int32 [B,P] updated IN PLACE -- per
    box the topk priors with their centre inside it whose prediction scores the largest t = conf^alpha * IoU^beta are
    selected, and every free prior some box selected goes to the box its prediction overlaps most.  alpha a multiple of
    0.5 in [0, 4], beta an int in [1, 16].  n_extra int32 [B] and thr float64 [B,G] (both optional) receive the number
    added per image and the t of each box's last selected prior.  Returns (match, n_extra, thr)."""
    B, P = match.shape
    G = gt_bboxes.shape[1]
    assert priors.shape == (P, 4) and decoded.shape == (B, P, 4) and conf.shape == (B, P) and gt_bboxes.shape == (B, G, 4)
    assert thr is None or (thr.is_cuda and thr.dtype == torch.float64 and thr.is_contiguous() and thr.shape == (B, G))
    halves = alpha * 2
    if isinstance(alpha, bool) or isinstance(beta, bool) or halves != int(halves) or beta != int(beta):
        raise ValueError("alpha must be a multiple of 0.5 and beta an int, got %r and %r" % (alpha, beta))
    _lib.check(_lib.lib().mbx_match_tal(_f32(priors).data_ptr(), _f32(decoded).data_ptr(), _f32(conf).data_ptr(),
                                        _f32(gt_bboxes).data_ptr(), _i32(num_gt_bboxes).data_ptr(),
                                        _i32(status).data_ptr(), int(topk), int(halves), int(beta), B, P, G,
                                        _i32(match).data_ptr(), None if n_extra is None else _i32(n_extra).data_ptr(),
                                        None if thr is None else thr.data_ptr(), _stream()), "mbx_match_tal")
    return match, n_extra, thr


def compute_assignments(locations, confidences, gt_bboxes, num_gt_bboxes, batch_size, alpha):
    """loss.py:8-53.  Same inputs/outputs as the py_func callback: returns
    [assignment_partitions int32 [B*P], stacked_gt_bboxes float32 [M,4]] (row order),
    and raises like the callback would (scipy ValueError -> TF UnknownError) on a bad cost matrix."""
    B = int(batch_size)
    loc = locations.reshape(B, -1, 4).contiguous()
    P = loc.shape[1]
    conf = confidences.reshape(B, P).contiguous()
    match, status = match_boxes(loc, conf, gt_bboxes.contiguous(), num_gt_bboxes.to(torch.int32).contiguous(), alpha)
    st = status.cpu()
    if int(st.max()) != 0:
        raise ValueError("compute_assignments: infeasible or non-finite cost matrix (status %s)" % st.tolist())
    part = (match >= 0).to(torch.int32).reshape(-1)
    b_idx, p_idx = torch.nonzero(match >= 0, as_tuple=True)           # row-major == ascending row order
    stacked = gt_bboxes[b_idx, match[b_idx, p_idx].long()].to(torch.float32)
    return [part, stacked]


def _focal_arguments(focal_gamma, focal_alpha):
    """None (off), or (gamma, w_pos, w_neg) as mbx_loss_fwd_bwd_focal takes them.  Raises ValueError on a bad value."""
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if focal_gamma is None:
        if focal_alpha is not None:
            raise ValueError("focal_alpha is given without focal_gamma")
        return None
    if not (number(focal_gamma) and 0.0 <= focal_gamma <= 10.0):
        raise ValueError("focal_gamma must be a number in [0, 10], got %r" % (focal_gamma,))
    if focal_alpha is None:
        return float(focal_gamma), 1.0, 1.0
    if not (number(focal_alpha) and 0.0 < focal_alpha < 1.0):
        raise ValueError("focal_alpha must be a number inside (0, 1), got %r" % (focal_alpha,))
    return float(focal_gamma), float(focal_alpha), 1.0 - float(focal_alpha)


LOC_BETA_DEFAULT = 0.1


def _loc_arguments(loc_loss, loc_beta):
    """None (off), or (loc_type, loc_beta) as mbx_loss_fwd_bwd_loc takes them.  Raises ValueError on a bad value."""
    if loc_loss is None:
        if loc_beta is not None:
            raise ValueError("loc_beta is given without loc_loss")
        return None
    if not (isinstance(loc_loss, str) and loc_loss in LOC_TYPES):
        raise ValueError("loc_loss must be one of %s, got %r" % (", ".join(LOC_TYPES), loc_loss))
    if loc_loss != "smooth_l1":
        if loc_beta is not None:
            raise ValueError("loc_beta goes with loc_loss 'smooth_l1' only, got it with %r" % (loc_loss,))
        return LOC_TYPES.index(loc_loss), 0.0
    if loc_beta is None:
        return LOC_TYPES.index(loc_loss), LOC_BETA_DEFAULT
    # the entry takes a float32: the value has to be finite and > 0 as one
    if not (isinstance(loc_beta, (int, float)) and not isinstance(loc_beta, bool)
            and 0.0 < ctypes.c_float(loc_beta).value < float("inf")):
        raise ValueError("loc_beta must be a finite number > 0 (as a float32), got %r" % (loc_beta,))
    return LOC_TYPES.index(loc_loss), float(loc_beta)


QUALITY_TARGETS = ("qfl", "varifocal")                       # MBX_QUALITY_QFL = 1, MBX_QUALITY_VFL = 2 (include/mbx.h)
QUALITY_NEG_WEIGHT_DEFAULT = {"qfl": 1.0, "varifocal": 0.75}  # the papers' settings


def _quality_arguments(quality_target, quality_gamma, quality_neg_weight):
    """None (off), or (quality, gamma, w_pos, w_neg) as mbx_loss_fwd_bwd_quality takes them.  Raises ValueError on a bad
    value."""
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if quality_target is None:
        for name, v in (("quality_gamma", quality_gamma), ("quality_neg_weight", quality_neg_weight)):
            if v is not None:
                raise ValueError("%s is given without quality_target" % name)
        return None
    if not (isinstance(quality_target, str) and quality_target in QUALITY_TARGETS):
        raise ValueError("quality_target must be one of %s, got %r" % (", ".join(QUALITY_TARGETS), quality_target))
    gamma = 2.0 if quality_gamma is None else quality_gamma
    if not (number(gamma) and 0.0 <= gamma <= 10.0):
        raise ValueError("quality_gamma must be a number in [0, 10], got %r" % (gamma,))
    if quality_target == "qfl" and 0.0 < gamma < 1.0:
        raise ValueError("quality_gamma must be 0 or >= 1 with quality_target 'qfl', got %r" % (gamma,))
    w_neg = QUALITY_NEG_WEIGHT_DEFAULT[quality_target] if quality_neg_weight is None else quality_neg_weight
    if not (number(w_neg) and 0.0 < ctypes.c_float(w_neg).value < float("inf")):
        raise ValueError("quality_neg_weight must be a finite number > 0 (as a float32), got %r" % (w_neg,))
    return QUALITY_TARGETS.index(quality_target) + 1, float(gamma), 1.0, float(w_neg)


IGNORE_SOURCES = ("prior", "prediction")


def _ignore_arguments(ignore_iou_threshold, ignore_source):
    """None (off), or (threshold, per_image) as mbx_match_ignore takes them.  Raises ValueError on a bad value."""
    if not (isinstance(ignore_source, str) and ignore_source in IGNORE_SOURCES):
        raise ValueError("ignore_source must be one of %s, got %r" % (", ".join(IGNORE_SOURCES), ignore_source))
    if ignore_iou_threshold is None:
        if ignore_source != "prior":
            raise ValueError("ignore_source is given without ignore_iou_threshold")
        return None
    v = ignore_iou_threshold
    # the entry takes a float32: the value has to be in (0, 1] as one
    if not (isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 < ctypes.c_float(v).value <= 1.0):
        raise ValueError("ignore_iou_threshold must be a number in (0, 1] (as a float32), got %r" % (v,))
    return float(v), int(ignore_source == "prediction")


class MultiboxLoss:
    """Fused decode + match + loss (+ gradients) with preallocated buffers (no allocation per step).

    neg_per_pos (an int >= 1; None = off, the reference's loss): hard-negative mining -- per image only the
    max(min_neg, neg_per_pos * positives) highest-scoring negatives count (mbx_loss_fwd_bwd_mined, include/mbx.h);
    their number per image is left in ``n_neg``.  What that does to AP on real data is not measured here.

    match_iou_threshold (a float in (0, 1]; None = off, the reference's bipartite match alone): threshold matching --
    behind mbx_match every prior still free goes to the box it overlaps most if that IoU is over the threshold
    (mbx_match_extend, include/mbx.h); the number added per image is left in ``n_extra``.  The loss, mined or not, reads
    the extended ``match``.  What that does to AP on real data is not measured here either.

    atss_topk (an int >= 1; None = off) with prior_levels (the list [0, ..., P] of where each pyramid level of the priors
    starts, required with it): ATSS matching in the place of threshold matching -- behind mbx_match every box takes the
    atss_topk priors nearest to its centre on every level as candidates, and the free ones at or over the mean plus the
    standard deviation of the candidates' IoUs whose centre lies in the box become its positives (mbx_match_atss,
    include/mbx.h); the number added per image is left in ``n_atss``, the thresholds in ``atss_thr``.  Not together with
    match_iou_threshold: both decide what a free prior becomes.  With k priors per cell sharing a centre, 9 reaches about
    two cells of a level at k = 5; the paper's nine locations are 9 * k.  What that does to AP on real data is not measured
    here either.

    tal_topk (an int >= 1, 13 in the paper; None = off) with tal_alpha (a multiple of 0.5 in [0, 4], default 1) and tal_beta
    (an int in [1, 16], default 6; both only with tal_topk): task-aligned matching (TOOD, Feng et al. 2021) in the place of
    threshold or ATSS matching -- behind mbx_match every box selects the tal_topk priors with their centre inside it whose
    PREDICTION scores the largest conf^alpha * IoU^beta, and a free prior some box selected becomes a positive of the box
    its prediction overlaps most (mbx_match_tal, include/mbx.h); the number added per image is left in ``n_tal``, the metric
    of each box's last selected prior in ``tal_thr``.  Not together with match_iou_threshold or atss_topk: each decides what
    a free prior becomes.  The bipartite match stays, so every box keeps one guaranteed prior while the predictions still
    overlap nothing; TOOD's normalised soft target is not part of it, quality_target supplies an IoU target.  What that
    does to AP on real data is not measured here either.

    focal_gamma (a float in [0, 10]; None = off, the reference's loss): the focal loss on the confidence term -- a
    positive's -log c is weighted by w^gamma and a counted negative's -log w by c^gamma (mbx_loss_fwd_bwd_focal,
    include/mbx.h).  focal_alpha (a float inside (0, 1); None = both sides weigh 1; only with focal_gamma) weighs the
    positives by alpha and the negatives by 1 - alpha.  With neg_per_pos the mined negatives are the ones counted, and the
    extended ``match`` is read as by the other two.  What that does to AP on real data is not measured here either.

    loc_loss (one of LOC_TYPES: "l2", "smooth_l1", "giou", "diou", "ciou"; None = off, the reference's L2 through the entry
    chosen above): the location term of a positive (mbx_loss_fwd_bwd_loc, include/mbx.h, the one entry for every
    combination with the three switches above; "l2" gives the reference's bytes through it).  loc_beta (a finite float > 0,
    default 0.1; only with "smooth_l1") is where smooth-L1 turns from quadratic to linear.  The match keeps the reference's
    L2-based cost.  location_loss_alpha's 1000 was sized for L2: with an IoU type, whose term is of order 1 per positive,
    pass your own.  What any of these does to AP on real data is not measured here either.

    quality_target ("qfl" or "varifocal"; None = off): an IoU-aware confidence target -- a positive trains its confidence
    towards the IoU of its prediction with its box, by the Quality Focal Loss or the Varifocal Loss
    (mbx_loss_fwd_bwd_quality, include/mbx.h, the one entry for every combination with loc_loss and neg_per_pos; w_pos = 1).
    quality_gamma (a float in [0, 10], under "qfl" 0 or >= 1; default 2) is the exponent of both sides, quality_neg_weight
    (finite and > 0; default 1 under "qfl", 0.75 under "varifocal") weighs the negatives; both only with the target.  Not
    together with focal_gamma / focal_alpha: each decides the confidence term.  The sum of the positives' IoUs and their
    number per image are left in ``q_stats`` ([B, 2] float64).  Scores trained this way estimate localisation quality as
    well as objectness.  What that does to AP on real data is not measured here either.

    ignore_iou_threshold (a float in (0, 1]; None = off): the ignore band -- behind the matching above every prior still
    free that overlaps some box of its image by at least the threshold is neither positive nor negative: no confidence
    loss, no gradient, no candidate and no positive for mining (mbx_match_ignore writes -2 into ``match``,
    mbx_loss_fwd_bwd_ignore, the one entry for every combination with the switches above, leaves those out; include/mbx.h);
    their number per image is left in ``n_ignored``.  ignore_source ("prior", the default, or "prediction"; only with the
    threshold) says whose overlap counts: the prior's own, or the decoded prediction's (YOLOv3's rule).  With
    match_iou_threshold and source "prior" the threshold must not be above it: no free prior overlaps a box by more.  What
    that does to AP on real data is not measured here either."""

    def __init__(self, bbox_priors, batch_size, max_num_bboxes, location_loss_alpha, device="cuda", neg_per_pos=None,
                 min_neg=0, match_iou_threshold=None, focal_gamma=None, focal_alpha=None, loc_loss=None, loc_beta=None,
                 atss_topk=None, prior_levels=None, quality_target=None, quality_gamma=None, quality_neg_weight=None,
                 ignore_iou_threshold=None, ignore_source="prior", tal_topk=None, tal_alpha=TAL_ALPHA_DEFAULT,
                 tal_beta=TAL_BETA_DEFAULT):
        self.tal = _tal_arguments(tal_topk, tal_alpha, tal_beta)
        if self.tal is not None and (match_iou_threshold is not None or atss_topk is not None):
            raise ValueError("tal_topk and %s are both given: each decides what a free prior becomes"
                             % ("match_iou_threshold" if match_iou_threshold is not None else "atss_topk"))
        self.focal = _focal_arguments(focal_gamma, focal_alpha)
        self.loc = _loc_arguments(loc_loss, loc_beta)
        self.quality = _quality_arguments(quality_target, quality_gamma, quality_neg_weight)
        self.ignore = _ignore_arguments(ignore_iou_threshold, ignore_source)
        if self.ignore is not None and match_iou_threshold is not None and not self.ignore[1] \
                and isinstance(match_iou_threshold, (int, float)) and self.ignore[0] > match_iou_threshold:
            raise ValueError("ignore_iou_threshold %r is above match_iou_threshold %r: no free prior overlaps a box by that "
                             "much, the band would be empty" % (ignore_iou_threshold, match_iou_threshold))
        if self.quality is not None and self.focal is not None:
            raise ValueError("quality_target and focal_gamma / focal_alpha are both given: each decides the confidence term")
        self.priors = torch.as_tensor(bbox_priors, dtype=torch.float32).to(device).contiguous()
        self.P = self.priors.shape[0]
        self.B, self.G, self.alpha = int(batch_size), int(max_num_bboxes), float(location_loss_alpha)
        f = dict(dtype=torch.float32, device=device)
        self.decoded = torch.empty((self.B, self.P, 4), **f)
        self.conf = torch.empty((self.B, self.P), **f)
        self.match = torch.empty((self.B, self.P), dtype=torch.int32, device=device)
        self.status = torch.zeros((self.B,), dtype=torch.int32, device=device)
        self.loss2 = torch.zeros((2,), **f)
        self.d_locs = torch.empty((self.B, self.P, 4), **f)
        self.d_logits = torch.empty((self.B, self.P), **f)
        self.neg_per_pos, self.min_neg, self.n_neg = neg_per_pos, min_neg, None
        mining = (0, 0, None)                                  # (neg_per_pos, min_neg, n_neg) as the entries take them
        if neg_per_pos is not None:
            self.n_neg = torch.zeros((self.B,), dtype=torch.int32, device=device)
            mining = (neg_per_pos, min_neg, self.n_neg.data_ptr())
        # the entry forward_backward calls, the arguments it has between the common ones and the workspace, its workspace
        l = _lib.lib()
        self.q_stats, self.n_ignored = None, None
        if self.ignore is not None:
            # the superset entry, whatever else is on: loc, quality and focal defaults filled in as the quality branch does
            self.n_ignored = torch.zeros((self.B,), dtype=torch.int32, device=device)
            if self.quality is not None:
                self.q_stats = torch.zeros((self.B, 2), dtype=torch.float64, device=device)
            confidence = self.quality or ((0,) + (self.focal or (0.0, 1.0, 1.0)))
            self.entry = "mbx_loss_fwd_bwd_ignore"
            self.entry_args = (self.loc or (0, 0.0)) + confidence + mining + \
                (None if self.q_stats is None else self.q_stats.data_ptr(),)
            ws_bytes = l.mbx_loss_ignore_workspace_bytes(self.B, self.P)
        elif self.quality is not None:
            self.q_stats = torch.zeros((self.B, 2), dtype=torch.float64, device=device)
            self.entry = "mbx_loss_fwd_bwd_quality"
            self.entry_args = (self.loc or (0, 0.0)) + self.quality + mining + (self.q_stats.data_ptr(),)
            ws_bytes = l.mbx_loss_quality_workspace_bytes(self.B, self.P)
        elif self.loc is not None:
            self.entry, self.entry_args = "mbx_loss_fwd_bwd_loc", self.loc + (self.focal or (0.0, 1.0, 1.0)) + mining
            ws_bytes = l.mbx_loss_loc_workspace_bytes(self.B, self.P)
        elif self.focal is not None:
            self.entry, self.entry_args = "mbx_loss_fwd_bwd_focal", self.focal + mining
            ws_bytes = l.mbx_loss_focal_workspace_bytes(self.B, self.P)
        elif neg_per_pos is not None:
            self.entry, self.entry_args = "mbx_loss_fwd_bwd_mined", mining
            ws_bytes = l.mbx_loss_mined_workspace_bytes(self.B, self.P)
        else:
            self.entry, self.entry_args = "mbx_loss_fwd_bwd", ()
            ws_bytes = l.mbx_loss_workspace_bytes(self.B)
        self.ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        self.match_iou_threshold, self.n_extra = match_iou_threshold, None
        if match_iou_threshold is not None:
            if not 0.0 < float(match_iou_threshold) <= 1.0:
                raise ValueError("match_iou_threshold must be in (0, 1], got %r" % (match_iou_threshold,))
            self.match_iou_threshold = float(match_iou_threshold)
            self.n_extra = torch.zeros((self.B,), dtype=torch.int32, device=device)
        self.atss_topk, self.prior_levels, self.n_atss, self.atss_thr = None, None, None, None
        if atss_topk is not None:
            if match_iou_threshold is not None:
                raise ValueError("atss_topk and match_iou_threshold are both given: each decides what a free prior becomes")
            if not (isinstance(atss_topk, int) and not isinstance(atss_topk, bool) and 1 <= atss_topk <= 2 ** 31 - 1):
                raise ValueError("atss_topk must be an int >= 1, got %r" % (atss_topk,))
            if prior_levels is None:
                raise ValueError("atss_topk needs prior_levels, the list [0, ..., P] of where each level of the priors starts")
            try:
                levels = [int(v) for v in prior_levels]
            except (TypeError, ValueError):
                raise ValueError("prior_levels must be a list of ints, got %r" % (prior_levels,))
            if not (2 <= len(levels) <= 9 and levels[0] == 0 and levels[-1] == self.P
                    and all(a < b for a, b in zip(levels, levels[1:]))):
                raise ValueError("prior_levels must hold 1 to 8 levels, start at 0, ascend strictly and end at the %d priors, "
                                 "got %r" % (self.P, levels))
            self._level_table, self._n_levels = _level_table(levels)
            verdict = l.mbx_match_atss_supported(self.P, self.G, self._n_levels, self._level_table, atss_topk)
            if verdict != 0:
                raise ValueError("atss_topk %d with prior_levels %r, %d priors and %d boxes an image: mbx_match_atss says %s"
                                 % (atss_topk, levels, self.P, self.G, l.mbx_status_string(verdict).decode()))
            self.atss_topk, self.prior_levels = atss_topk, levels
            self.n_atss = torch.zeros((self.B,), dtype=torch.int32, device=device)
            self.atss_thr = torch.zeros((self.B, self.G), dtype=torch.float64, device=device)
        elif prior_levels is not None:
            raise ValueError("prior_levels is given without atss_topk")
        self.tal_topk, self.n_tal, self.tal_thr = None, None, None
        if self.tal is not None:
            verdict = l.mbx_match_tal_supported(self.P, self.G, self.tal[0])
            if verdict != 0:
                raise ValueError("tal_topk %d with %d priors and %d boxes an image: mbx_match_tal says %s"
                                 % (self.tal[0], self.P, self.G, l.mbx_status_string(verdict).decode()))
            self.tal_topk = self.tal[0]
            self.n_tal = torch.zeros((self.B,), dtype=torch.int32, device=device)
            self.tal_thr = torch.zeros((self.B, self.G), dtype=torch.float64, device=device)

    def forward_backward(self, raw_locs, logits, gt_bboxes, num_gt_bboxes, grad_scale=1.0, conf_is_logit=True):
        """raw_locs [B,P,4], logits [B,P] f32 -> (loss2 [2] = {location_loss, confidence_loss}, d_locs, d_logits)."""
        l, s = _lib.lib(), _stream()
        B, P, G = self.B, self.P, self.G
        assert raw_locs.shape == (B, P, 4) and logits.numel() == B * P and gt_bboxes.shape == (B, G, 4)
        if conf_is_logit:
            _lib.check(l.mbx_decode_conf(_f32(raw_locs).data_ptr(), _f32(logits).data_ptr(), self.priors.data_ptr(),
                                         B, P, SMALL_EPSILON, self.decoded.data_ptr(), self.conf.data_ptr(), s),
                       "mbx_decode_conf")
        else:
            _lib.check(l.mbx_decode_conf(_f32(raw_locs).data_ptr(), None, self.priors.data_ptr(), B, P, 0.0,
                                         self.decoded.data_ptr(), None, s), "mbx_decode_conf")
            torch.add(logits.reshape(B, P), SMALL_EPSILON, out=self.conf)        # loss.py:74
        _lib.check(l.mbx_match(self.decoded.data_ptr(), self.conf.data_ptr(), _f32(gt_bboxes).data_ptr(),
                               _i32(num_gt_bboxes).data_ptr(), self.alpha, B, P, G, self.match.data_ptr(),
                               self.status.data_ptr(), None, 0, s), "mbx_match")
        if self.match_iou_threshold is not None:
            _lib.check(l.mbx_match_extend(self.priors.data_ptr(), gt_bboxes.data_ptr(), num_gt_bboxes.data_ptr(),
                                          self.status.data_ptr(), self.match_iou_threshold, B, P, G,
                                          self.match.data_ptr(), self.n_extra.data_ptr(), s), "mbx_match_extend")
        if self.atss_topk is not None:
            _lib.check(l.mbx_match_atss(self.priors.data_ptr(), self._level_table, self._n_levels, gt_bboxes.data_ptr(),
                                        num_gt_bboxes.data_ptr(), self.status.data_ptr(), self.atss_topk, B, P, G,
                                        self.match.data_ptr(), self.n_atss.data_ptr(), self.atss_thr.data_ptr(), s),
                       "mbx_match_atss")
        if self.tal is not None:
            _lib.check(l.mbx_match_tal(self.priors.data_ptr(), self.decoded.data_ptr(), self.conf.data_ptr(),
                                       gt_bboxes.data_ptr(), num_gt_bboxes.data_ptr(), self.status.data_ptr(), *self.tal,
                                       B, P, G, self.match.data_ptr(), self.n_tal.data_ptr(), self.tal_thr.data_ptr(), s),
                       "mbx_match_tal")
        if self.ignore is not None:
            boxes = self.decoded if self.ignore[1] else self.priors
            _lib.check(l.mbx_match_ignore(boxes.data_ptr(), self.ignore[1], gt_bboxes.data_ptr(), num_gt_bboxes.data_ptr(),
                                          self.status.data_ptr(), self.ignore[0], B, P, G, self.match.data_ptr(),
                                          self.n_ignored.data_ptr(), s), "mbx_match_ignore")
        common = (self.decoded.data_ptr(), _f32(logits).data_ptr(), int(bool(conf_is_logit)), gt_bboxes.data_ptr(),
                  self.match.data_ptr(), self.alpha, float(grad_scale), B, P, G, self.loss2.data_ptr(), self.d_locs.data_ptr(),
                  self.d_logits.data_ptr())
        _lib.check(getattr(l, self.entry)(*common, *self.entry_args, self.ws.data_ptr(), self.ws.numel(), s), self.entry)
        return self.loss2, self.d_locs, self.d_logits


def add_loss(locations, confidences, batched_bboxes, batched_num_bboxes, bbox_priors, location_loss_alpha):
    """loss.py:55-116 (forward value): locations [B,P,4] raw residuals, confidences [B,P,1] sigmoid outputs.
    Returns (location_loss, confidence_loss) as 0-d CUDA tensors."""
    B = locations.shape[0]
    m = MultiboxLoss(bbox_priors, B, batched_bboxes.shape[1], location_loss_alpha, device=locations.device)
    loss2, _, _ = m.forward_backward(locations.contiguous(), confidences.reshape(B, -1).contiguous(),
                                     batched_bboxes.to(torch.float32).contiguous(),
                                     batched_num_bboxes.to(torch.int32).contiguous(), conf_is_logit=False)
    st = m.status.cpu()
    if int(st.max()) != 0:
        raise ValueError("add_loss: matching failed (status %s)" % st.tolist())
    return loss2[0].clone(), loss2[1].clone()
