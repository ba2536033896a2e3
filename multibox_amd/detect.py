"""Detection post-processing -- host mirror of the reference's detect.py loop on libmbx.

``postprocess`` replaces the per-patch numpy loop detect.py:408-443 with one launch of
``mbx_decode_filter_topk``; ``extract_patches`` keeps the reference's offsets and
restrictions (detect.py:20-72).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import records as REC


def extract_patches(image, patch_dims, strides, non_edge_restriction=0.1):
    """detect.py:20-72: same return list [patches, offsets(y,x), restrictions, count]."""
    H, W = image.shape[:2]
    ph, pw = patch_dims
    sh, sw = strides
    hs = list(range(0, H - ph + 1, sh))
    ws = list(range(0, W - pw + 1, sw))
    n = len(hs) * len(ws)
    patches = np.zeros((n, ph, pw, 3), np.float32)
    offs = np.zeros((n, 2), np.int32)
    res = np.zeros((n, 4), np.float32)
    i = 0
    for h in hs:
        for w in ws:
            patches[i] = image[h:h + ph, w:w + pw]
            offs[i] = (h, w)
            res[i] = (0.0 if w == 0 else non_edge_restriction, 0.0 if h == 0 else non_edge_restriction,
                      1.0 if w + pw == W else 1.0 - non_edge_restriction,
                      1.0 if h + ph == H else 1.0 - non_edge_restriction)
            i += 1
    return [patches, offs, res, np.int32(n)]


PATCH_META_DTYPE = np.dtype([("offset_y", "<i4"), ("offset_x", "<i4"), ("patch_h", "<i4"), ("patch_w", "<i4"),
                             ("image_h", "<i4"), ("image_w", "<i4"), ("is_flipped", "<i4"), ("max_to_keep", "<i4"),
                             ("restrictions", "<f4", (4,))])
assert PATCH_META_DTYPE.itemsize == ctypes.sizeof(_lib.PatchMeta)      # mbx_patch_meta (include/mbx.h)


def make_patch_meta(offsets, dims, is_flipped, restrictions, max_to_keep, image_hw, device="cuda"):
    """Pack the per-patch columns fetched at detect.py:398-406 into mbx_patch_meta[B] on the device (whole columns at a
    time: a Python loop over 256 patches was 1.5 ms of the detect loop's main thread)."""
    B = len(offsets)
    m = np.zeros(B, PATCH_META_DTYPE)
    off, dm, hw = np.asarray(offsets).reshape(B, 2), np.asarray(dims).reshape(B, 2), np.asarray(image_hw).reshape(B, 2)
    m["offset_y"], m["offset_x"] = off[:, 0], off[:, 1]
    m["patch_h"], m["patch_w"] = dm[:, 0], dm[:, 1]
    m["image_h"], m["image_w"] = hw[:, 0], hw[:, 1]
    m["is_flipped"] = np.asarray(is_flipped).reshape(B, -1)[:, 0]
    m["max_to_keep"] = np.asarray(max_to_keep).reshape(B, -1)[:, 0]
    m["restrictions"] = np.asarray(restrictions, np.float32).reshape(B, 4)
    return torch.from_numpy(m.view(np.uint8).reshape(-1)).to(device)


class DetectPostprocess:
    """Preallocated outputs for B patches x k_max detections (k_max >= every max_to_keep)."""

    def __init__(self, bbox_priors, batch_size, k_max=200, device="cuda", nms_iou=None):
        """nms_iou: None (the reference: no NMS, detect.py:408-443) or an IoU threshold for the optional greedy
        per-patch NMS stage (mbx_nms, row N1)."""
        self.nms_iou = None if nms_iou is None else float(nms_iou)
        self.priors = torch.as_tensor(bbox_priors, dtype=torch.float32).to(device).contiguous()
        self.P, self.B, self.K = self.priors.shape[0], int(batch_size), int(k_max)
        self.boxes = torch.empty((self.B, self.K, 4), dtype=torch.float64, device=device)
        self.scores = torch.empty((self.B, self.K), dtype=torch.float32, device=device)
        self.index = torch.empty((self.B, self.K), dtype=torch.int32, device=device)
        self.count = torch.empty((self.B,), dtype=torch.int32, device=device)

    def __call__(self, raw_locs, confs, meta):
        """raw_locs [B,P,4] f32, confs [B,P] f32 (sigmoid outputs), meta uint8 tensor from make_patch_meta."""
        B, P = self.B, self.P
        assert raw_locs.shape == (B, P, 4) and confs.numel() == B * P and meta.numel() == B * ctypes.sizeof(_lib.PatchMeta)
        assert raw_locs.is_contiguous() and confs.is_contiguous() and raw_locs.dtype == confs.dtype == torch.float32
        _lib.check(_lib.lib().mbx_decode_filter_topk(raw_locs.data_ptr(), confs.data_ptr(), self.priors.data_ptr(),
                                                     meta.data_ptr(), B, P, self.K, self.boxes.data_ptr(),
                                                     self.scores.data_ptr(), self.index.data_ptr(),
                                                     self.count.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "mbx_decode_filter_topk")
        if self.nms_iou is not None:
            _lib.check(_lib.lib().mbx_nms(self.boxes.data_ptr(), self.scores.data_ptr(), self.index.data_ptr(),
                                          self.count.data_ptr(), B, self.K, self.nms_iou,
                                          torch.cuda.current_stream().cuda_stream), "mbx_nms")
        return self.boxes, self.scores, self.index, self.count


def results_to_json_records(boxes, scores, count, image_ids):
    """detect.py:438-443: list of {"image_id", "bbox", "score"} in patch order."""
    as_np = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()
    boxes, scores, count = as_np(boxes), as_np(scores), as_np(count)
    out = []
    for b in range(boxes.shape[0]):
        n = int(count[b])
        image_id = image_ids[b]
        out.extend({"image_id": image_id, "bbox": bb, "score": sc}
                   for bb, sc in zip(boxes[b, :n].tolist(), scores[b, :n].tolist()))
    return out


from .records import results_to_json_text, batch_chunk, records_to_json      # noqa: E402,F401  (torch-free: run in worker processes)


# ----------------------------------------------------------------------------- per-image merge (not in the reference)
class ImageMerger:
    """All candidates of one image, from all its patches, ordered by score, de-duplicated by greedy NMS across patches and
    cut to max_detections (mbx_merge_detections, one workgroup per image).  Fed with the HOST copies of the per-patch
    stage's output, batch by batch in stream order -- the same path for one rank and for many; the rows of one image
    are adjacent, an image may straddle batches.  iou_threshold None or inf: no suppression, top-N per image.
    vote_iou None: the kept boxes are the kept candidates' own (mbx_merge_detections, as ever).  A float in (0, 1]: box
    voting (mbx_merge_detections_voted) -- the same kept list and scores, every kept box replaced by the score-weighted
    mean of all candidates of its image with IoU >= vote_iou against it.  An image above 16 384 candidates is still cut
    to its best 16 384 on the host first, and only those vote.
    soft None: greedy suppression, as above.  ("linear" | "gaussian", sigma, min_score) (records.merge_soft_nms checks it):
    Soft-NMS (mbx_merge_detections_soft) -- an overlapping candidate's score is lowered instead of the candidate deleted,
    the scores that come out are the decayed ones, in pick order.  Linear takes iou_threshold as its threshold (None is a
    ValueError), gaussian ignores it; vote_iou is passed through.  The host-side cut above 16 384 candidates comes first.
    wbf None: one of the forms above.  ("avg" | "max", iou_threshold, min_score, expected_views) (records.merge_wbf checks
    it): weighted boxes fusion (mbx_merge_detections_wbf) -- the candidates are clustered against the running fused box of
    each cluster, and the clusters come out: the score-weighted mean box, and a score that falls when fewer than
    expected_views candidates agree.  It has its own threshold (iou_threshold is not read) and composes with neither
    voting nor Soft-NMS: vote_iou and soft must be None.  The host-side cut above 16 384 candidates comes first."""

    def __init__(self, k_max, max_detections, iou_threshold, device="cuda", flush_images=256, vote_iou=None, soft=None,
                 wbf=None):
        self.K, self.max_det = int(k_max), int(max_detections)
        self.thr = float("inf") if iou_threshold is None else float(iou_threshold)
        self.vote_iou = REC.merge_vote_iou(vote_iou)
        self.soft = None if soft is None else REC.merge_soft_nms(*soft)
        if self.soft is not None and self.soft[0] == REC.SOFT_NMS_METHODS["linear"] and (iou_threshold is None or self.thr != self.thr):
            raise ValueError("linear Soft-NMS needs an IoU threshold (scores decay above it), not %r" % (iou_threshold,))
        self.wbf = None if wbf is None else REC.merge_wbf(*wbf)
        if self.wbf is not None and (self.vote_iou is not None or self.soft is not None):
            raise ValueError("weighted boxes fusion (wbf) composes with neither box voting (vote_iou) nor Soft-NMS (soft): "
                             "both must be None, not %r and %r" % (vote_iou, soft))
        self._ws = None                                     # the fusion's workspace: kept between launches, grows when it must
        self.device, self.flush_images = device, max(1, int(flush_images))
        self.stream = torch.cuda.Stream(device=device)      # its uploads and launches do not queue behind the detect loop
        self._rows, self._ids, self._runs = [], [], 0
        self._out = []                                      # (ids, boxes, scores, count) per launch
        self._warned = False

    def add(self, boxes, scores, count, image_ids):
        """boxes [B,K,4] f64, scores [B,K] f32, count [B] i32 (host arrays of one batch; copied), image_ids [B]."""
        boxes, scores, count = (np.array(boxes, np.float64), np.array(scores, np.float32), np.array(count, np.int32))
        assert boxes.shape == (len(count), self.K, 4) and scores.shape == (len(count), self.K) == (len(image_ids), self.K)
        for i in image_ids:
            if not self._ids or i != self._ids[-1]:
                self._runs += 1
            self._ids.append(i)
        self._rows.append((boxes, scores, count))
        if self._runs - 1 >= self.flush_images:             # every image but the one the stream is still in
            self._flush(final=False)

    def _flush(self, final):
        if not self._ids:
            return
        ids, image_rows = REC.group_rows(self._ids)
        n_img = len(ids) if final else len(ids) - 1
        if n_img == 0:
            return
        end = int(image_rows[n_img])
        boxes, scores, count = (np.concatenate([r[j] for r in self._rows]) for j in range(3))
        self._rows = [(boxes[end:], scores[end:], count[end:])] if end < len(count) else []
        self._ids, self._runs = self._ids[end:], len(ids) - n_img
        ids, image_rows = ids[:n_img], image_rows[:n_img + 1].copy()
        boxes, scores, count = boxes[:end], scores[:end], np.clip(count[:end], 0, self.K)
        per_image = np.add.reduceat(np.concatenate([count, [0]]).astype(np.int64), image_rows[:-1])   # (no image is empty of rows)
        if (per_image > REC.MERGE_MAX_CANDIDATES).any():
            if not self._warned:
                print("WARNING: an image has more than %d candidates; merging its best %d (warned once per run)"
                      % (REC.MERGE_MAX_CANDIDATES, REC.MERGE_MAX_CANDIDATES), flush=True)
                self._warned = True
            parts, new_rows = [], [0]
            for i in range(n_img):
                a, b = int(image_rows[i]), int(image_rows[i + 1])
                part = (boxes[a:b], scores[a:b], count[a:b])
                if per_image[i] > REC.MERGE_MAX_CANDIDATES:
                    part = REC.repack_rows(part[0], part[1], REC.best_candidates(part[1], part[2]), self.K)
                parts.append(part)
                new_rows.append(new_rows[-1] + len(part[2]))
            boxes, scores, count = (np.concatenate([p[j] for p in parts]) for j in range(3))
            image_rows = np.array(new_rows, np.int32)
        assert len(count) * self.K < 2 ** 31
        with torch.cuda.stream(self.stream):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            d_boxes, d_scores, d_count, d_rows = up(boxes), up(scores), up(count.astype(np.int32)), up(image_rows.astype(np.int32))
            o_boxes = torch.empty((n_img, self.max_det, 4), dtype=torch.float64, device=self.device)
            o_scores = torch.empty((n_img, self.max_det), dtype=torch.float32, device=self.device)
            o_src = torch.empty((n_img, self.max_det), dtype=torch.int32, device=self.device)
            o_count = torch.empty((n_img,), dtype=torch.int32, device=self.device)
            o_status = torch.empty((n_img,), dtype=torch.int32, device=self.device)
            call = "mbx_merge_detections" if self.vote_iou is None else "mbx_merge_detections_voted"
            if self.wbf is not None:
                call = "mbx_merge_detections_wbf"
                conf, thr, min_score, views = self.wbf
                need = _lib.lib().mbx_merge_wbf_workspace(len(count), self.K)
                if self._ws is None or self._ws.numel() < need:
                    self._ws = None                         # (the old one goes before the new one comes)
                    self._ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
                o_votes = torch.empty((n_img, self.max_det), dtype=torch.int32, device=self.device)
                _lib.check(_lib.lib().mbx_merge_detections_wbf(d_boxes.data_ptr(), d_scores.data_ptr(), d_count.data_ptr(),
                                                               d_rows.data_ptr(), len(count), n_img, self.K, self.max_det,
                                                               conf, thr, min_score, views, o_boxes.data_ptr(),
                                                               o_scores.data_ptr(), o_src.data_ptr(), o_count.data_ptr(),
                                                               o_status.data_ptr(), o_votes.data_ptr(), self._ws.data_ptr(),
                                                               self._ws.numel(), self.stream.cuda_stream), call)
            elif self.soft is not None:
                call = "mbx_merge_detections_soft"
                method, sigma, min_score = self.soft
                o_votes = None if self.vote_iou is None else torch.empty((n_img, self.max_det), dtype=torch.int32, device=self.device)
                _lib.check(_lib.lib().mbx_merge_detections_soft(d_boxes.data_ptr(), d_scores.data_ptr(), d_count.data_ptr(),
                                                                d_rows.data_ptr(), n_img, self.K, self.max_det, method,
                                                                self.thr if method == 1 else 0.0, sigma, min_score,
                                                                0.0 if self.vote_iou is None else self.vote_iou,
                                                                o_boxes.data_ptr(), o_scores.data_ptr(), o_src.data_ptr(),
                                                                o_count.data_ptr(), o_status.data_ptr(),
                                                                None if o_votes is None else o_votes.data_ptr(),
                                                                self.stream.cuda_stream), call)
            elif self.vote_iou is None:
                _lib.check(_lib.lib().mbx_merge_detections(d_boxes.data_ptr(), d_scores.data_ptr(), d_count.data_ptr(),
                                                           d_rows.data_ptr(), n_img, self.K, self.max_det, self.thr,
                                                           o_boxes.data_ptr(), o_scores.data_ptr(), o_src.data_ptr(),
                                                           o_count.data_ptr(), o_status.data_ptr(), self.stream.cuda_stream),
                           "mbx_merge_detections")
            else:
                o_votes = torch.empty((n_img, self.max_det), dtype=torch.int32, device=self.device)
                _lib.check(_lib.lib().mbx_merge_detections_voted(d_boxes.data_ptr(), d_scores.data_ptr(), d_count.data_ptr(),
                                                                 d_rows.data_ptr(), n_img, self.K, self.max_det, self.thr,
                                                                 self.vote_iou, o_boxes.data_ptr(), o_scores.data_ptr(),
                                                                 o_src.data_ptr(), o_count.data_ptr(), o_status.data_ptr(),
                                                                 o_votes.data_ptr(), self.stream.cuda_stream),
                           "mbx_merge_detections_voted")
            status = o_status.cpu().numpy()
            if status.any():
                raise _lib.MbxError("%s: status %d for image %r" % (call, int(status.max()), ids[int(np.argmax(status != 0))]))
            self._out.append((ids, o_boxes.cpu().numpy(), o_scores.cpu().numpy(), o_count.cpu().numpy()))

    def finish(self):
        """Flush the rest (the last image included): (ids, boxes [N,max_det,4], scores [N,max_det], count [N]), images in
        stream order, each image's detections in kept order."""
        self._flush(final=True)
        out, self._out = self._out, []
        if not out:
            return ([], np.zeros((0, self.max_det, 4), np.float64), np.zeros((0, self.max_det), np.float32), np.zeros((0,), np.int32))
        return ([i for o in out for i in o[0]],) + tuple(np.concatenate([o[j] for o in out]) for j in (1, 2, 3))


# ----------------------------------------------------------------------------- multi-GPU detect
# Patches are independent (per-patch loop, detect.py:408): ranks take disjoint batches, NO collective on the data
# path; at the end rank 0 concatenates the per-rank result lists into the one JSON of detect.py:458-460.
def shard_batches(batches, rank, world):
    """Yield (global batch index, batch) for the batches this rank owns: batch i goes to rank i % world, so every
    rank keeps the single-process batching (tf.train.batch order, detect.py:283-292) and the merge below can
    restore the single-process order of the results."""
    for i, b in enumerate(batches):
        if i % world == rank:
            yield i, b


def merge_results(per_rank):
    """per_rank: one list per rank of (global batch index, [records]).  Returns the records in batch order --
    exactly what one process would have written."""
    tagged = [t for part in per_rank for t in part]
    tagged.sort(key=lambda t: t[0])
    assert [t[0] for t in tagged] == sorted(set(t[0] for t in tagged)), "a batch was processed by two ranks"
    return [r for _, recs in tagged for r in recs]


def gather_results(local, group=None):
    """Rank 0 gets merge_results() of every rank's [(batch index, records)]; other ranks get None.  Host-side
    object gather (gloo or RCCL-backed group both work); single process: just the merge."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return merge_results([local])
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    parts = [None] * world if rank == 0 else None
    dist.gather_object(local, parts, dst=0, group=group)
    return merge_results(parts) if rank == 0 else None
