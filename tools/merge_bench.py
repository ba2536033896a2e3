"""mbx_merge_detections timing on seeded candidates (multibox_amd.synth.merge_candidates): device events around 20 launches
after 3 warm-ups, for (a) 256 images of the config.yaml.example VGA plan (44 rows per image: 1 x 200 + 43 x 50 candidates,
k_max 200, max_det 100, IoU 0.5) and (b) 64 images x 80 rows x 200 candidates (max_det 300, IoU 0.3).
--vote_iou X also times mbx_merge_detections_voted (box voting at vote IoU X: the merge launch + the vote launch) on the
same inputs: five rounds of 20 plain and 20 voted launches in turn, the median round of each.
--soft linear|gaussian (one or both) also times mbx_merge_detections_soft (Soft-NMS: linear above the shape's IoU, gaussian
at sigma 0.5, min_score 0.001) on the same inputs, and with --vote_iou each method with the vote launch behind it: three
rounds of 20 launches of the plain merge and of every variant in turn, the median round of each.
usage: python tools/merge_bench.py [--vote_iou X] [--soft linear|gaussian ...]"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--vote_iou", type=float, default=None)
ap.add_argument("--soft", nargs="+", choices=["linear", "gaussian"], default=[])
args = ap.parse_args()
g.build()
from multibox_amd import _lib
from multibox_amd.synth import merge_candidates

l = _lib.lib()
for name, I, rows, K, n_obj, max_det, thr in (("a: VGA plan", 256, 44, 200, 8, 100, 0.5), ("b: 80 full rows", 64, 80, 200, 40, 300, 0.3)):
    count = np.full((I, rows), 200, np.int32)
    if rows == 44:
        count[:, 1:] = 50
    boxes, scores, count, image_rows = merge_candidates(seed=rows, I=I, rows_per_image=(rows, rows), K=K, n_obj=n_obj,
                                                        count=count.reshape(-1))
    d_b, d_s, d_c, d_r = (torch.from_numpy(a).cuda() for a in (boxes, scores, count, image_rows))
    o_b = torch.empty((I, max_det, 4), dtype=torch.float64, device="cuda")
    o_s = torch.empty((I, max_det), dtype=torch.float32, device="cuda")
    o_i = torch.empty((I, max_det), dtype=torch.int32, device="cuda")
    o_c, o_st = (torch.empty((I,), dtype=torch.int32, device="cuda") for _ in range(2))
    s = torch.cuda.current_stream().cuda_stream
    call = lambda: _lib.check(l.mbx_merge_detections(d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), I, K, max_det,
                                                     thr, o_b.data_ptr(), o_s.data_ptr(), o_i.data_ptr(), o_c.data_ptr(),
                                                     o_st.data_ptr(), s), "mbx_merge_detections")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 20 * 1e3
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    us = timed(call)
    sha = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in (o_b, o_s, o_i, o_c, o_st))).hexdigest()[:12]
    n_cand = int(count.sum())
    print("%s: I=%d rows=%d k_max=%d max_det=%d iou=%.1f: %.1f us/launch  %.0f images/s  %.3g candidates/s  kept %d..%d  "
          "status_max %d  outputs sha %s" % (name, I, rows, K, max_det, thr, us, I / us * 1e6, n_cand / us * 1e6, int(o_c.min()),
                                             int(o_c.max()), int(o_st.max()), sha), flush=True)
    o_v = torch.empty((I, max_det), dtype=torch.int32, device="cuda")
    if args.soft:
        def soft_call(method, vote):
            return lambda: _lib.check(l.mbx_merge_detections_soft(
                d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), I, K, max_det, {"linear": 1, "gaussian": 2}[method],
                thr, 0.5, 0.001, vote or 0.0, o_b.data_ptr(), o_s.data_ptr(), o_i.data_ptr(), o_c.data_ptr(), o_st.data_ptr(),
                o_v.data_ptr() if vote else None, s), "mbx_merge_detections_soft")
        variants = [("plain", call)] + [("soft " + m, soft_call(m, None)) for m in args.soft]
        if args.vote_iou is not None:
            variants += [("soft %s + vote %.2f" % (m, args.vote_iou), soft_call(m, args.vote_iou)) for m in args.soft]
        kept = {}
        for label, fn in variants:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            kept[label] = "kept %d..%d" % (int(o_c.min()), int(o_c.max()))
        rounds = {label: [] for label, _ in variants}
        for _ in range(3):
            for label, fn in variants:
                rounds[label].append(timed(fn))
        base = float(np.median(rounds["plain"]))
        for label, _ in variants:
            t = rounds[label]
            print("%s: %s: %.1f us/launch (rounds %s)  %.2f x plain  %s" % (name[0], label, float(np.median(t)),
                  " ".join("%.1f" % v for v in t), float(np.median(t)) / base, kept[label]), flush=True)
    if args.vote_iou is None:
        continue
    voted = lambda: _lib.check(l.mbx_merge_detections_voted(d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), I, K,
                                                            max_det, thr, args.vote_iou, o_b.data_ptr(), o_s.data_ptr(),
                                                            o_i.data_ptr(), o_c.data_ptr(), o_st.data_ptr(), o_v.data_ptr(), s),
                               "mbx_merge_detections_voted")
    for _ in range(3):
        voted()
    torch.cuda.synchronize()
    t_plain, t_voted = [], []
    for _ in range(5):
        t_plain.append(timed(call))
        t_voted.append(timed(voted))
    sha_v = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in (o_b, o_s, o_i, o_c, o_st, o_v))).hexdigest()[:12]
    votes = o_v.cpu().numpy()[np.arange(max_det)[None, :] < o_c.cpu().numpy()[:, None]]
    fmt = lambda t: "%.1f us/launch (rounds %s)" % (float(np.median(t)), " ".join("%.1f" % v for v in t))
    print("%s: vote_iou=%.2f: plain %s  voted %s  vote launch +%.1f us  votes per kept box min %d median %d max %d  "
          "outputs sha %s" % (name[0], args.vote_iou, fmt(t_plain), fmt(t_voted), float(np.median(t_voted) - np.median(t_plain)),
                              int(votes.min()), int(np.median(votes)), int(votes.max()), sha_v), flush=True)
