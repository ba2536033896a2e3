"""COCO metric timing on seeded input (multibox_amd.synth.coco_eval_set: a 299-pixel frame, 1-13 gts and 100 detections per
image -- jittered gts plus random boxes -- as eval.py hands them over):
  (a) mbx_coco_match alone, device events around 20 launches after 3 warm-ups;
  (b) cocoeval.evaluate_bbox_device end to end (pack + upload + kernel + download + accumulate), with its split;
  (c) cocoeval.evaluate_bbox (the pure-Python metric eval.py runs without --device_metric) on the same input.
(b) and (c) alternate three times in this one process, after one untimed (b) that loads the library; their twelve numbers
and lines must be equal before anything is printed.  --big times (a) and (b) alone at a validation-set size.
usage: python tools/coco_match_bench.py [--images 500] [--big 5000]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as g

g.build()
from multibox_amd import _lib, cocoeval as CE
from multibox_amd.synth import coco_eval_set

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=500, help="size at which evaluate_bbox is timed too (it must finish within a minute)")
ap.add_argument("--big", type=int, default=5000, help="size at which only the device path is timed (0 = skip)")
args = ap.parse_args()
l = _lib.lib()


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def kernel_alone(packed):
    I, A, T = len(packed.img_ids), len(CE.AREA_RNG), len(CE.IOU_THRS)
    d_dt, d_dr, d_gt, d_gr = (torch.from_numpy(a.reshape(-1)).cuda() for a in (packed.dt, packed.dt_rows, packed.gt, packed.gt_rows))
    o_m = torch.empty((I, A, T, CE.MAX_DET), dtype=torch.int16, device="cuda")
    o_i = torch.empty((I, A, T, CE.MAX_DET), dtype=torch.uint8, device="cuda")
    o_n = torch.empty((I, A), dtype=torch.int32, device="cuda")
    o_s = torch.empty((I,), dtype=torch.int32, device="cuda")
    thrs, rng = np.ascontiguousarray(CE.IOU_THRS, np.float64), np.ascontiguousarray(CE.AREA_RNG, np.float64)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda: _lib.check(l.mbx_coco_match(d_dt.data_ptr(), d_dr.data_ptr(), d_gt.data_ptr(), d_gr.data_ptr(), I, thrs.ctypes.data,
                                               T, rng.ctypes.data, A, o_m.data_ptr(), o_i.data_ptr(), o_n.data_ptr(), o_s.data_ptr(), s),
                              "mbx_coco_match")
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 20 * 1e3, int(o_s.max()), int((o_m >= 0).sum())


def device_split(gt, dt):
    packed, t_pack = clock(lambda: CE.pack(gt, dt))
    m, t_match = clock(lambda: CE.match_device(packed))
    out, t_acc = clock(lambda: CE.accumulate(packed, *m))
    return packed, out, (t_pack, t_match, t_acc)


for I, with_host in ((args.images, True), (args.big, False)):
    if I <= 0:
        continue
    gt, dt = coco_eval_set(1, I, n_gt=(1, 13), n_dt=(100, 100), score_levels=64)
    packed, out, _ = device_split(gt, dt)                                 # untimed: library load, first launch
    us, status_max, n_matched = kernel_alone(packed)
    print("I=%d images, %d gts, %d detections" % (I, len(gt), len(dt)))
    print("(a) mbx_coco_match alone: %.1f us/launch  %.3g images/s  status_max %d  matched slots %d" % (us, I / us * 1e6, status_max, n_matched))
    dev, host, splits = [], [], []
    for _ in range(3):
        (d_out, t_d) = clock(lambda: CE.evaluate_bbox_device(gt, dt))
        dev.append(t_d)
        splits.append(device_split(gt, dt)[2])
        assert d_out == out
        if with_host:
            h_out, t_h = clock(lambda: CE.evaluate_bbox(gt, dt))
            host.append(t_h)
            assert tuple(h_out) == tuple(d_out), "evaluate_bbox_device and evaluate_bbox disagree"
    print("(b) evaluate_bbox_device end to end: " + "  ".join("%.3f s" % t for t in dev))
    print("    its split (separate runs) pack / match_device / accumulate: " +
          "  ".join("%.3f / %.3f / %.3f s" % s for s in splits))
    if with_host:
        print("(c) evaluate_bbox (host):            " + "  ".join("%.3f s" % t for t in host))
        print("    slowest (b) %.3f s vs fastest (c) %.3f s: %.1fx; stats equal, AP %.6f" % (max(dev), min(host), min(host) / max(dev), out[0][0]))
    else:
        print("    (c) not timed at this size; AP %.6f" % out[0][0])
    sys.stdout.flush()
