"""Synthetic inputs of the benchmark / tests: the reference has no generator, so the
shapes follow its input contract (inputs.py:340-351): images [B,S,S,3] float32 in [-1,1], ground
truth [B,G,4] zero-padded x1,y1,x2,y2 in [0,1], counts [B] int32."""
import numpy as np


def synthetic_batch(batch, size=299, max_num_bboxes=13, seed=0):
    rng = np.random.RandomState(seed)
    images = rng.uniform(-1.0, 1.0, (batch, size, size, 3)).astype(np.float32)
    rng = np.random.RandomState(seed + 1)
    n = rng.randint(0, max_num_bboxes + 1, batch).astype(np.int32)      # includes images without boxes
    gt = np.zeros((batch, max_num_bboxes, 4), np.float32)
    for b in range(batch):
        xy = rng.uniform(0, 0.7, (n[b], 2))
        wh = rng.uniform(0.05, 0.3, (n[b], 2))
        gt[b, :n[b], :2] = xy
        gt[b, :n[b], 2:] = xy + wh
    return images, gt, n


DEFAULT_ASPECT_RATIOS = {5: [1.0, 2.0, 3.0, 1.0 / 2.0, 1.0 / 3.0],
                         7: [1.0, 2.0, 3.0, 1.0 / 2.0, 1.0 / 3.0, 1.5, 1.0 / 1.5]}


def merge_candidates(seed, I, rows_per_image, K, n_obj, tie_levels=64, unrelated=0.3, count=None):
    """Seeded input of the per-image merge (mbx_merge_detections): I images of rows_per_image = (lo, hi) rows of K slots.
    Every image has n_obj objects; a slot holds a jittered copy of one of them or, with probability `unrelated`, an
    unrelated box; scores are quantised to 1 / tie_levels (ties in every image) and sorted within a row; `count` per row is
    random in [0, K] (or the given constant).  Returns boxes [R,K,4] f64, scores [R,K] f32, count [R] i32, image_rows [I+1]."""
    rng = np.random.RandomState(seed)
    rows = rng.randint(rows_per_image[0], rows_per_image[1] + 1, I)
    image_rows = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    R = int(image_rows[-1])
    boxes, scores = np.zeros((R, K, 4)), np.zeros((R, K), np.float32)
    cnt = rng.randint(0, K + 1, R).astype(np.int32)
    for i in range(I):
        c, wh = rng.uniform(0.15, 0.85, (n_obj, 2)), rng.uniform(0.05, 0.3, (n_obj, 2))
        for r in range(image_rows[i], image_rows[i + 1]):
            o = rng.randint(0, n_obj, K)
            jit = rng.normal(0, 0.01, (K, 4))
            bx = np.clip(np.stack([c[o, 0] - wh[o, 0] / 2 + jit[:, 0], c[o, 1] - wh[o, 1] / 2 + jit[:, 1],
                                   c[o, 0] + wh[o, 0] / 2 + jit[:, 2], c[o, 1] + wh[o, 1] / 2 + jit[:, 3]], 1), 0, 1)
            rnd = rng.rand(K) < unrelated
            rb = np.sort(rng.rand(K, 2, 2), axis=1).reshape(K, 4)[:, [0, 2, 1, 3]]
            bx[rnd] = rb[rnd]
            sc = (np.floor(rng.rand(K) * tie_levels) / tie_levels).astype(np.float32)
            boxes[r], scores[r] = bx, -np.sort(-sc)
    if count is not None:
        cnt = np.broadcast_to(np.asarray(count, np.int32), (R,)).copy()
    return boxes, scores, cnt, image_rows


def coco_eval_set(seed, I, n_gt=(0, 13), n_dt=(0, 130), size=299, quantum=0.5, score_levels=8, counts=None):
    """Seeded input of the COCO metric (cocoeval.evaluate_bbox / evaluate_bbox_device): I images in a size-pixel frame with
    n_gt = (lo, hi) ground-truth boxes (sides from a few pixels to most of the frame, so every area range is met) and
    n_dt = (lo, hi) detections: jittered copies of the image's gts and, for one in three (or without gts), random boxes.
    Coordinates are multiples of `quantum` pixels and scores take `score_levels` distinct values (0 = continuous scores),
    so IoU ties and score ties occur (one gt in seven
    repeats an earlier one of its image).  `counts`: the (gts, detections) of each image instead of random ones.  Returns (gt_annotations, pred_annotations) as eval.py builds them."""
    rng = np.random.RandomState(seed)
    q = lambda v: np.round(np.asarray(v, np.float64) / quantum) * quantum
    gts, dts = [], []
    for i in range(I):
        img_id = 1000 + 3 * i
        ng, nd = rng.randint(n_gt[0], n_gt[1] + 1), rng.randint(n_dt[0], n_dt[1] + 1)
        if counts is not None:
            ng, nd = counts[i]
        wh = q(np.exp(rng.uniform(np.log(4.0), np.log(0.8 * size), (ng, 2))))
        xy = q(rng.uniform(0, 1, (ng, 2)) * (size - wh))
        for j in range(1, ng):
            if rng.rand() < 0.15:                                         # the same object annotated twice: equal IoUs
                o = rng.randint(j)
                xy[j], wh[j] = xy[o], wh[o]
        for (x, y), (w, h) in zip(xy.tolist(), wh.tolist()):
            gts.append({"id": len(gts) + 1, "image_id": img_id, "category_id": 1, "area": w * h, "bbox": [x, y, w, h], "iscrowd": 0})
        for _ in range(nd):
            if ng and rng.rand() < 2.0 / 3.0:
                o = rng.randint(ng)
                x, y, w, h = q(np.concatenate([xy[o], wh[o]]) + rng.choice([-2.0, -0.5, 0.0, 0.0, 0.5, 2.0], 4) * np.tile(wh[o], 2) / 16)
            else:
                w, h = q(np.exp(rng.uniform(np.log(4.0), np.log(0.8 * size), 2)))
                x, y = q(rng.uniform(0, 1, 2) * (size - np.array([w, h])))
            s = (1 + rng.randint(score_levels)) / (score_levels + 1.0) if score_levels else rng.rand()
            dts.append([img_id, float(x), float(y), float(max(w, quantum)), float(max(h, quantum)), float(s), 1])
    return gts, dts
