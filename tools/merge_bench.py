"""mbx_merge_detections timing on seeded candidates (multibox_amd.synth.merge_candidates): device events around 20 launches
after 3 warm-ups, for (a) 256 images of the config.yaml.example VGA plan (44 rows per image: 1 x 200 + 43 x 50 candidates,
k_max 200, max_det 100, IoU 0.5) and (b) 64 images x 80 rows x 200 candidates (max_det 300, IoU 0.3).
usage: python tools/merge_bench.py"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as g

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
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        call()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / 20 * 1e3
    sha = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in (o_b, o_s, o_i, o_c, o_st))).hexdigest()[:12]
    n_cand = int(count.sum())
    print("%s: I=%d rows=%d k_max=%d max_det=%d iou=%.1f: %.1f us/launch  %.0f images/s  %.3g candidates/s  kept %d..%d  "
          "status_max %d  outputs sha %s" % (name, I, rows, K, max_det, thr, us, I / us * 1e6, n_cand / us * 1e6, int(o_c.min()),
                                             int(o_c.max()), int(o_st.max()), sha), flush=True)
