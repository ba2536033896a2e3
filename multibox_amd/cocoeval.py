"""COCO bounding-box AP / AR -- the metric step of the reference's eval.py:212-246.

The reference hands its top-100 boxes per image to pycocotools' COCOeval (iouType 'bbox', useCats = 0) and logs the
twelve summary numbers.  pycocotools is a third-party dependency that is absent here, so this restates its published
algorithm (cocoeval.py: evaluateImg / accumulate / summarize) for the case the reference uses: one category, no
crowd annotations.  "Parity unpinned": there is no pycocotools in this image to check against; the tests pin the
behaviour on hand-computed cases.

evaluate_bbox(gt, dt) with
  gt: list of {"image_id", "bbox": [x, y, w, h], "area", ["iscrowd": 0]}          (eval.py:176-186)
  dt: array-like rows [image_id, x, y, w, h, score, category]                      (eval.py:166-173)
returns the 12 statistics in COCOeval.stats order and the summary lines in its print format.
"""
from __future__ import annotations

import collections
import sys

import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RNG = [(0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DETS = [1, 10, 100]


def _iou_xywh(d, g):
    """IoU matrix [len(d), len(g)] of xywh boxes (maskUtils.iou with iscrowd = 0)."""
    if len(d) == 0 or len(g) == 0:
        return np.zeros((len(d), len(g)))
    dx0, dy0, dx1, dy1 = d[:, 0:1], d[:, 1:2], d[:, 0:1] + d[:, 2:3], d[:, 1:2] + d[:, 3:4]
    gx0, gy0, gx1, gy1 = g[:, 0], g[:, 1], g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    iw = np.clip(np.minimum(dx1, gx1) - np.maximum(dx0, gx0), 0, None)
    ih = np.clip(np.minimum(dy1, gy1) - np.maximum(dy0, gy0), 0, None)
    inter = iw * ih
    union = d[:, 2:3] * d[:, 3:4] + (g[:, 2] * g[:, 3])[None] - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)


def _evaluate_img(dt, gt, a_rng, max_det):
    """cocoeval.evaluateImg: dt rows [x,y,w,h,score] (any order), gt rows [x,y,w,h,area].  Returns
    (scores, matched [T,D] bool, det_ignore [T,D] bool, number of non-ignored gt)."""
    g_ig = ~((gt[:, 4] >= a_rng[0]) & (gt[:, 4] <= a_rng[1])) if len(gt) else np.zeros(0, bool)
    g_order = np.argsort(g_ig, kind="mergesort")                     # non-ignored first
    gt, g_ig = gt[g_order], g_ig[g_order]
    d_order = np.argsort(-dt[:, 4], kind="mergesort")[:max_det] if len(dt) else np.zeros(0, int)
    dt = dt[d_order]
    ious = _iou_xywh(dt[:, :4], gt[:, :4])
    T, D, G = len(IOU_THRS), len(dt), len(gt)
    dtm = -np.ones((T, D), int)
    gtm = -np.ones((T, G), int)
    dt_ig = np.zeros((T, D), bool)
    for ti, t in enumerate(IOU_THRS):
        for di in range(D):
            iou, m = min(t, 1 - 1e-10), -1
            for gi in range(G):
                if gtm[ti, gi] >= 0:
                    continue                                          # already matched (no crowd gt here)
                if m > -1 and not g_ig[m] and g_ig[gi]:
                    break                                             # matched to a regular gt: stop at the ignored ones
                if ious[di, gi] < iou:
                    continue
                iou, m = ious[di, gi], gi
            if m == -1:
                continue
            dt_ig[ti, di] = g_ig[m]
            dtm[ti, di] = m
            gtm[ti, m] = di
    d_area = dt[:, 2] * dt[:, 3]
    out_of_range = (d_area < a_rng[0]) | (d_area > a_rng[1])
    dt_ig = dt_ig | ((dtm == -1) & out_of_range[None, :])
    return dt[:, 4], dtm >= 0, dt_ig, int((~g_ig).sum())


def evaluate_bbox(gt_annotations, pred_annotations):
    pred = np.asarray(pred_annotations, dtype=np.float64).reshape(-1, 7) if len(pred_annotations) else np.zeros((0, 7))
    gt_by_img, dt_by_img = {}, {}
    for a in gt_annotations:
        x, y, w, h = a["bbox"]
        gt_by_img.setdefault(a["image_id"], []).append([x, y, w, h, a.get("area", w * h)])
    for r in pred:
        dt_by_img.setdefault(int(r[0]), []).append([r[1], r[2], r[3], r[4], r[5]])
    img_ids = sorted(set(gt_by_img) | set(dt_by_img))
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, A, M))
    recall = -np.ones((T, A, M))
    for ai, a_rng in enumerate(AREA_RNG):
        per_img = []
        for i in img_ids:
            g = np.asarray(gt_by_img.get(i, []), np.float64).reshape(-1, 5)
            d = np.asarray(dt_by_img.get(i, []), np.float64).reshape(-1, 5)
            if len(g) == 0 and len(d) == 0:
                continue
            per_img.append(_evaluate_img(d, g, a_rng, MAX_DETS[-1]))
        for mi, max_det in enumerate(MAX_DETS):
            if not per_img:
                continue
            scores = np.concatenate([e[0][:max_det] for e in per_img])
            order = np.argsort(-scores, kind="mergesort")
            dtm = np.concatenate([e[1][:, :max_det] for e in per_img], axis=1)[:, order]
            dig = np.concatenate([e[2][:, :max_det] for e in per_img], axis=1)[:, order]
            npig = sum(e[3] for e in per_img)
            if npig == 0:
                continue
            tps = np.cumsum(dtm & ~dig, axis=1).astype(np.float64)
            fps = np.cumsum(~dtm & ~dig, axis=1).astype(np.float64)
            for ti in range(T):
                tp, fp = tps[ti], fps[ti]
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                recall[ti, ai, mi] = rc[-1] if nd else 0
                pr = pr.tolist()
                for k in range(nd - 1, 0, -1):
                    if pr[k] > pr[k - 1]:
                        pr[k - 1] = pr[k]
                q = np.zeros(R)
                inds = np.searchsorted(rc, REC_THRS, side="left")
                for ri, pi in enumerate(inds):
                    if pi < nd:
                        q[ri] = pr[pi]
                precision[ti, :, ai, mi] = q

    def summarize(ap, iou_thr=None, area="all", max_det=100):
        ai, mi = AREA_LBL.index(area), MAX_DETS.index(max_det)
        s = precision[:, :, ai, mi] if ap else recall[:, ai, mi]
        if iou_thr is not None:
            s = s[np.where(np.isclose(IOU_THRS, iou_thr))[0]]
        v = float(np.mean(s[s > -1])) if (s > -1).any() else -1.0
        title, typ = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
        iou_s = "%0.2f:%0.2f" % (IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else "%0.2f" % iou_thr
        return v, " %-18s %s @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f" % (title, typ, iou_s, area, max_det, v)
    spec = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100), (1, None, "medium", 100),
            (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10), (0, None, "all", 100), (0, None, "small", 100),
            (0, None, "medium", 100), (0, None, "large", 100)]
    out = [summarize(*sp) for sp in spec]
    return [v for v, _ in out], [line for _, line in out]


# ---------------------------------------------------------------------------------------------------------------------
# The same metric with the matching and the accumulation on the GPU (mbx_coco_match, mbx_coco_accumulate, include/mbx.h):
# evaluate_bbox_device = pack -> match_device(on_device=True) -> accumulate_device -> _summarize.  evaluate_bbox above stays
# the oracle and the vectorised numpy accumulate_tables the reference of the device tables (and the path for sizes the
# kernels refuse); every array here holds exactly the float64 values evaluate_bbox builds, the kernels work on integers
# and repeat its divisions, and the twelve numbers come out bit for bit.
MAX_DET = 100                                                             # MBX_COCO_MAX_DET == MAX_DETS[-1]
MAX_GT = 128                                                              # MBX_COCO_MAX_GT
ACC_MAX_ND = 4194304                                                      # MBX_COCO_ACC_MAX_ND
ACC_CHUNK = 256                                                           # MBX_COCO_ACC_CHUNK
ACC_SORT_TILE = 1024                                                      # MBX_COCO_ACC_SORT_TILE
MBX_ERR_UNSUPPORTED = -2

Packed = collections.namedtuple("Packed", "img_ids dt dt_rows gt gt_rows")


def pack(gt_annotations, pred_annotations):
    """The inputs of mbx_coco_match: img_ids sorted; dt [ND,5] x,y,w,h,score, per image by score descending (stable) and
    cut to MAX_DETS[-1]; gt [NG,5] x,y,w,h,area, per image in annotation order; dt_rows / gt_rows [I+1] int32."""
    pred = np.asarray(pred_annotations, dtype=np.float64).reshape(-1, 7) if len(pred_annotations) else np.zeros((0, 7))
    g_ids, g_rows = [], []
    for a in gt_annotations:
        x, y, w, h = a["bbox"]
        g_ids.append(a["image_id"])
        g_rows.append([x, y, w, h, a.get("area", w * h)])
    d_uniq, d_inv = np.unique(pred[:, 0].astype(np.int64), return_inverse=True)            # int(r[0]) truncates too
    img_ids = sorted(set(g_ids) | set(d_uniq.tolist()))
    index = {i: k for k, i in enumerate(img_ids)}
    I = len(img_ids)
    g_img = np.array([index[i] for i in g_ids], np.int64)
    gt = np.asarray(g_rows, np.float64).reshape(-1, 5)[np.argsort(g_img, kind="mergesort")]
    d_img = np.array([index[i] for i in d_uniq.tolist()], np.int64)[d_inv.reshape(-1)]
    order = np.lexsort((-pred[:, 5], d_img))                               # image, then score descending; stable
    d_img = d_img[order]
    first = np.concatenate([[0], np.cumsum(np.bincount(d_img, minlength=I))])
    keep = np.arange(len(order)) - first[d_img] < MAX_DETS[-1]
    dt = np.ascontiguousarray(pred[order][keep][:, 1:6])
    rows = lambda img: np.concatenate([[0], np.cumsum(np.bincount(img, minlength=I))]).astype(np.int32)
    return Packed(img_ids, dt, rows(d_img[keep]), np.ascontiguousarray(gt), rows(g_img))


def _image(packed, i):
    return packed.dt[packed.dt_rows[i]:packed.dt_rows[i + 1]], packed.gt[packed.gt_rows[i]:packed.gt_rows[i + 1]]


def match_host(packed, images=None):
    """_evaluate_img on every image (or on `images`) and area range: matched [I,A,T,MAX_DET] bool, ignore (uint8, same
    shape), n_gt_counted [I,A] int32.  The oracle of match_device and its path for the images the kernel refuses."""
    I, A, T = len(packed.img_ids), len(AREA_RNG), len(IOU_THRS)
    matched = np.zeros((I, A, T, MAX_DET), bool)
    ignore = np.zeros((I, A, T, MAX_DET), np.uint8)
    n_gt_counted = np.zeros((I, A), np.int32)
    for i in range(I) if images is None else images:
        d, g = _image(packed, i)
        for ai, a_rng in enumerate(AREA_RNG):
            _, m, ig, n = _evaluate_img(d, g, a_rng, MAX_DETS[-1])
            matched[i, ai, :, :len(d)], ignore[i, ai, :, :len(d)], n_gt_counted[i, ai] = m, ig, n
    return matched, ignore, n_gt_counted


def _match_rows(dt, gt, a_rng):
    """WHICH gt each detection of _evaluate_img takes, as the row in annotation order ([T,D] int16, -1 = none), by the
    rule mbx_coco_match implements: among the free gts with IoU >= the start value, the in-range ones before the others,
    the largest IoU, of equal ones the later."""
    ious = _iou_xywh(dt[:, :4], gt[:, :4])
    in_rng = (gt[:, 4] >= a_rng[0]) & (gt[:, 4] <= a_rng[1])
    rows = -np.ones((len(IOU_THRS), len(dt)), np.int16)
    for ti, t in enumerate(IOU_THRS):
        free = np.ones(len(gt), bool)
        for di in range(len(dt)):
            for cls in (in_rng, ~in_rng):
                c = free & cls & (ious[di] >= min(t, 1 - 1e-10))
                if c.any():
                    j = len(gt) - 1 - int(np.argmax(np.where(c, ious[di], -1.0)[::-1]))
                    rows[ti, di], free[j] = j, False
                    break
    return rows


def match_device(packed, on_device=False):
    """mbx_coco_match on the current device: match [I,A,T,MAX_DET] int16 (gt row in annotation order or -1), ignore uint8,
    n_gt_counted [I,A] int32.  Images the kernel refuses (status 1: more than MAX_GT gts) come from match_host; input
    that is not finite goes to match_host altogether.  on_device: the three as device tensors, without the download
    (only the status and the refused images' rows cross the bus); numpy arrays still where the host computed everything."""
    I, A, T = len(packed.img_ids), len(AREA_RNG), len(IOU_THRS)
    if not (np.isfinite(packed.dt).all() and np.isfinite(packed.gt).all()):
        print("WARNING: non-finite box or score: COCO matching runs on the host", file=sys.stderr, flush=True)
        matched, ignore, n_gt_counted = match_host(packed)
        match = -np.ones(matched.shape, np.int16)
        for i in range(I):
            d, g = _image(packed, i)
            for ai, a_rng in enumerate(AREA_RNG):
                match[i, ai, :, :len(d)] = _rows_checked(d, g, a_rng, matched[i, ai, :, :len(d)], strict=False)
        return match, ignore, n_gt_counted
    if I == 0:
        return np.zeros((0, A, T, MAX_DET), np.int16), np.zeros((0, A, T, MAX_DET), np.uint8), np.zeros((0, A), np.int32)
    import torch
    from . import _lib
    dev = lambda a: torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, a.dtype)).cuda()
    d_dt, d_dr, d_gt, d_gr = dev(packed.dt), dev(packed.dt_rows), dev(packed.gt), dev(packed.gt_rows)
    o_m = torch.empty((I, A, T, MAX_DET), dtype=torch.int16, device="cuda")
    o_i = torch.empty((I, A, T, MAX_DET), dtype=torch.uint8, device="cuda")
    o_n = torch.empty((I, A), dtype=torch.int32, device="cuda")
    o_s = torch.empty((I,), dtype=torch.int32, device="cuda")
    thrs = np.ascontiguousarray(IOU_THRS, np.float64)
    rng = np.ascontiguousarray(AREA_RNG, np.float64)
    _lib.check(_lib.lib().mbx_coco_match(d_dt.data_ptr(), d_dr.data_ptr(), d_gt.data_ptr(), d_gr.data_ptr(), I,
                                         thrs.ctypes.data, T, rng.ctypes.data, A, o_m.data_ptr(), o_i.data_ptr(),
                                         o_n.data_ptr(), o_s.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "mbx_coco_match")
    if on_device:
        refused = np.nonzero(o_s.cpu().numpy())[0]
        if len(refused):                                                  # the kernel wrote -1 / 0 / 0 for these
            matched, h_ig, h_n = match_host(packed, refused)
            rows = -np.ones((len(refused), A, T, MAX_DET), np.int16)
            for k, i in enumerate(refused):
                d, g = _image(packed, i)
                for ai, a_rng in enumerate(AREA_RNG):
                    rows[k, ai, :, :len(d)] = _rows_checked(d, g, a_rng, matched[i, ai, :, :len(d)])
            where = torch.from_numpy(refused.astype(np.int64)).cuda()
            o_m[where] = torch.from_numpy(rows).cuda()
            o_i[where] = torch.from_numpy(np.ascontiguousarray(h_ig[refused])).cuda()
            o_n[where] = torch.from_numpy(np.ascontiguousarray(h_n[refused])).cuda()
        return o_m, o_i, o_n
    match, ignore, n_gt_counted, status = (t.cpu().numpy() for t in (o_m, o_i, o_n, o_s))
    refused = np.nonzero(status)[0]
    if len(refused):
        matched, h_ig, h_n = match_host(packed, refused)
        for i in refused:
            d, g = _image(packed, i)
            ignore[i], n_gt_counted[i] = h_ig[i], h_n[i]
            for ai, a_rng in enumerate(AREA_RNG):
                match[i, ai, :, :len(d)] = _rows_checked(d, g, a_rng, matched[i, ai, :, :len(d)])
    return match, ignore, n_gt_counted


def _rows_checked(d, g, a_rng, matched, strict=True):
    """_match_rows, held against _evaluate_img's `matched`.  A NaN box compares differently in the two; such an image
    (strict = False) then gets row 0 wherever it is matched: the metric only reads match >= 0."""
    rows = _match_rows(d, g, a_rng)
    if not np.array_equal(rows >= 0, matched):
        if strict:
            raise AssertionError("cocoeval._match_rows disagrees with _evaluate_img")
        rows = np.where(matched, 0, -1).astype(np.int16)
    return rows


def _summarize(precision, recall):
    """The summary of evaluate_bbox (COCOeval.summarize) on its precision [T,R,A,M] / recall [T,A,M] tables."""
    def summarize(ap, iou_thr=None, area="all", max_det=100):
        ai, mi = AREA_LBL.index(area), MAX_DETS.index(max_det)
        s = precision[:, :, ai, mi] if ap else recall[:, ai, mi]
        if iou_thr is not None:
            s = s[np.where(np.isclose(IOU_THRS, iou_thr))[0]]
        v = float(np.mean(s[s > -1])) if (s > -1).any() else -1.0
        title, typ = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
        iou_s = "%0.2f:%0.2f" % (IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else "%0.2f" % iou_thr
        return v, " %-18s %s @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f" % (title, typ, iou_s, area, max_det, v)
    spec = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100), (1, None, "medium", 100),
            (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10), (0, None, "all", 100), (0, None, "small", 100),
            (0, None, "medium", 100), (0, None, "large", 100)]
    out = [summarize(*sp) for sp in spec]
    return [v for v, _ in out], [line for _, line in out]


def accumulate_tables(packed, matched, ignore, n_gt_counted):
    """COCOeval.accumulate on the arrays of match_host / match_device (`matched` bool, or the int16 `match` whose >= 0 it
    is): precision [T,R,A,M] and recall [T,A,M], by the same sort, sums and divisions as evaluate_bbox.  The definition
    and oracle of mbx_coco_accumulate."""
    matched = np.asarray(matched)
    if matched.dtype != bool:
        matched = matched >= 0
    ignore = np.asarray(ignore).astype(bool)
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, A, M))
    recall = -np.ones((T, A, M))
    I = len(packed.img_ids)
    n_dt = np.diff(packed.dt_rows)
    d_img = np.repeat(np.arange(I), n_dt)                                 # images in sorted-id order, as evaluate_bbox
    d_slot = np.arange(len(d_img)) - packed.dt_rows[:-1].astype(np.int64)[d_img]
    for mi, max_det in enumerate(MAX_DETS):
        if I == 0:
            continue
        sel = np.nonzero(d_slot < max_det)[0]
        sel = sel[np.argsort(-packed.dt[sel, 4], kind="mergesort")]
        img, slot = d_img[sel], d_slot[sel]
        nd = len(sel)
        for ai in range(A):
            npig = int(n_gt_counted[:, ai].sum())
            if npig == 0:
                continue
            dtm, dig = matched[img, ai, :, slot].T, ignore[img, ai, :, slot].T                 # [T, nd]
            tps = np.cumsum(dtm & ~dig, axis=1).astype(np.float64)
            fps = np.cumsum(~dtm & ~dig, axis=1).astype(np.float64)
            rc = tps / npig
            pr = tps / (fps + tps + np.spacing(1))
            pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]      # pr[k-1] = max(pr[k-1], pr[k]) from the right
            recall[:, ai, mi] = rc[:, -1] if nd else 0
            for ti in range(T):
                inds = np.searchsorted(rc[ti], REC_THRS, side="left")
                ok = inds < nd
                q = np.zeros(R)
                q[ok] = pr[ti, inds[ok]]
                precision[ti, :, ai, mi] = q
    return precision, recall


def accumulate(packed, matched, ignore, n_gt_counted):
    """The second half of evaluate_bbox (COCOeval.accumulate + summarize) on the arrays of match_host / match_device: the
    same twelve floats."""
    return _summarize(*accumulate_tables(packed, matched, ignore, n_gt_counted))


class AccumulateUnsupported(Exception):
    """mbx_coco_accumulate returned MBX_ERR_UNSUPPORTED (more than ACC_MAX_ND detections)."""


def accumulate_device(packed, match, ignore, n_gt_counted):
    """accumulate_tables by mbx_coco_accumulate on the current device: (precision, recall) as numpy arrays, bit for bit.
    match / ignore / n_gt_counted are match_device's outputs, device tensors (on_device=True) or numpy arrays."""
    import torch
    from . import _lib
    I, A, T = len(packed.img_ids), len(AREA_RNG), len(IOU_THRS)
    R, M = len(REC_THRS), len(MAX_DETS)
    nd = int(packed.dt_rows[-1]) if I else 0
    assert len(packed.dt) == nd

    def dev(a, dtype):
        if isinstance(a, torch.Tensor):
            assert a.is_cuda and a.dtype == dtype and a.is_contiguous()
            return a if a.numel() else torch.zeros(1, dtype=dtype, device="cuda")
        a = np.ascontiguousarray(a)
        if a.dtype == bool and dtype == torch.int16:                      # match_host's `matched`
            a = np.where(a, 0, -1).astype(np.int16)
        t = torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, a.dtype))
        assert t.dtype == dtype
        return t.cuda()
    d_m, d_i, d_n = dev(match, torch.int16), dev(ignore, torch.uint8), dev(n_gt_counted, torch.int32)
    assert d_m.numel() >= I * A * T * MAX_DET and d_i.numel() >= I * A * T * MAX_DET and d_n.numel() >= I * A
    d_dt, d_dr = dev(packed.dt, torch.float64), dev(packed.dt_rows, torch.int32)
    l = _lib.lib()
    ws_bytes = l.mbx_coco_accumulate_workspace(nd, T, A, M)
    if nd > ACC_MAX_ND:
        raise AccumulateUnsupported("%d detections > %d" % (nd, ACC_MAX_ND))
    if ws_bytes == 0:
        raise _lib.MbxError("mbx_coco_accumulate_workspace refuses ND=%d T=%d A=%d M=%d" % (nd, T, A, M))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    o_p = torch.empty((T, R, A, M), dtype=torch.float64, device="cuda")
    o_r = torch.empty((T, A, M), dtype=torch.float64, device="cuda")
    thrs = np.ascontiguousarray(REC_THRS, np.float64)
    mds = np.ascontiguousarray(MAX_DETS, np.int32)
    rc = l.mbx_coco_accumulate(d_dt.data_ptr(), d_dr.data_ptr(), I, d_m.data_ptr(), d_i.data_ptr(), d_n.data_ptr(), T, A,
                               thrs.ctypes.data, R, mds.ctypes.data, M, o_p.data_ptr(), o_r.data_ptr(), ws.data_ptr(),
                               ws_bytes, torch.cuda.current_stream().cuda_stream)
    if rc == MBX_ERR_UNSUPPORTED:
        raise AccumulateUnsupported("mbx_coco_accumulate: unsupported size")
    _lib.check(rc, "mbx_coco_accumulate")
    return o_p.cpu().numpy(), o_r.cpu().numpy()


def evaluate_bbox_device(gt_annotations, pred_annotations):
    """evaluate_bbox with the matching and the accumulation on the GPU: the same twelve floats and lines.  Non-finite
    input takes the host path altogether; more detections than mbx_coco_accumulate takes are accumulated by numpy."""
    packed = pack(gt_annotations, pred_annotations)
    if not (np.isfinite(packed.dt).all() and np.isfinite(packed.gt).all()):
        return accumulate(packed, *match_device(packed))                  # (warns; match_host inside)
    m = match_device(packed, on_device=True)
    try:
        return _summarize(*accumulate_device(packed, *m))
    except AccumulateUnsupported:
        return accumulate(packed, *(t.cpu().numpy() if hasattr(t, "cpu") else t for t in m))
