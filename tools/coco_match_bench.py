"""COCO metric timing on seeded input (multibox_amd.synth.coco_eval_set: a 299-pixel frame, 1-13 gts and 100 detections per
image -- jittered gts plus random boxes -- as eval.py hands them over):
  (a) mbx_coco_match alone, device events around 20 launches after 3 warm-ups;
  (a') mbx_coco_accumulate alone, likewise (the call reads one integer back before it launches, so the events span that wait);
  (b) cocoeval.evaluate_bbox_device end to end (pack + upload + both kernels + download of the two tables + summary), with
      its split pack / match_device(on_device=True) / accumulate_device (upload of dt, launches, download of the tables),
      and beside it the split of the path it replaces: match_device with its download / numpy accumulate_tables; the two
      alternate, and their tables must be equal; also the download of match and ignore alone, which (b) no longer makes;
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


def accumulate_alone(packed, m):
    I, A, T, R, M = len(packed.img_ids), len(CE.AREA_RNG), len(CE.IOU_THRS), len(CE.REC_THRS), len(CE.MAX_DETS)
    d_dt, d_dr = (torch.from_numpy(a.reshape(-1)).cuda() for a in (packed.dt, packed.dt_rows))
    ws_bytes = l.mbx_coco_accumulate_workspace(len(packed.dt), T, A, M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    o_p = torch.empty((T, R, A, M), dtype=torch.float64, device="cuda")
    o_r = torch.empty((T, A, M), dtype=torch.float64, device="cuda")
    thrs, mds = np.ascontiguousarray(CE.REC_THRS, np.float64), np.ascontiguousarray(CE.MAX_DETS, np.int32)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda: _lib.check(l.mbx_coco_accumulate(d_dt.data_ptr(), d_dr.data_ptr(), I, m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr(),
                                                    T, A, thrs.ctypes.data, R, mds.ctypes.data, M, o_p.data_ptr(), o_r.data_ptr(),
                                                    ws.data_ptr(), ws_bytes, s), "mbx_coco_accumulate")
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 20 * 1e3, ws_bytes


def device_split(gt, dt):
    packed, t_pack = clock(lambda: CE.pack(gt, dt))
    m, t_match = clock(lambda: CE.match_device(packed, on_device=True))
    tables, t_acc = clock(lambda: CE.accumulate_device(packed, *m))
    return packed, m, tables, (t_pack, t_match, t_acc)


def host_split(packed):
    m, t_match = clock(lambda: CE.match_device(packed))
    tables, t_acc = clock(lambda: CE.accumulate_tables(packed, *m))
    return tables, (t_match, t_acc)


for I, with_host in ((args.images, True), (args.big, False)):
    if I <= 0:
        continue
    gt, dt = coco_eval_set(1, I, n_gt=(1, 13), n_dt=(100, 100), score_levels=64)
    packed, m, tables, _ = device_split(gt, dt)                           # untimed: library load, first launch
    out = CE._summarize(*tables)
    us, status_max, n_matched = kernel_alone(packed)
    us_acc, ws_bytes = accumulate_alone(packed, m)
    print("I=%d images, %d gts, %d detections" % (I, len(gt), len(dt)))
    print("(a) mbx_coco_match alone: %.1f us/launch  %.3g images/s  status_max %d  matched slots %d" % (us, I / us * 1e6, status_max, n_matched))
    print("(a') mbx_coco_accumulate alone: %.1f us/call  workspace %.1f MB" % (us_acc, ws_bytes / 1e6))
    dev, host, splits, h_splits, downloads = [], [], [], [], []
    for _ in range(3):
        (d_out, t_d) = clock(lambda: CE.evaluate_bbox_device(gt, dt))
        dev.append(t_d)
        _, m, d_tables, split = device_split(gt, dt)
        h_tables, h_split = host_split(packed)
        downloads.append(clock(lambda: [t.cpu() for t in m[:2]])[1])
        splits.append(split)
        h_splits.append(h_split)
        assert d_out == out
        assert all(np.array_equal(a, b) for a, b in zip(d_tables, h_tables)), "accumulate_device and accumulate_tables disagree"
        if with_host:
            h_out, t_h = clock(lambda: CE.evaluate_bbox(gt, dt))
            host.append(t_h)
            assert tuple(h_out) == tuple(d_out), "evaluate_bbox_device and evaluate_bbox disagree"
    print("(b) evaluate_bbox_device end to end: " + "  ".join("%.3f s" % t for t in dev))
    print("    its split (separate runs) pack / match_device(on_device) / accumulate_device: " +
          "  ".join("%.3f / %.4f / %.4f s" % s for s in splits))
    print("    the path it replaces, match_device with download / numpy accumulate_tables:   " +
          "  ".join("%.4f / %.4f s" % s for s in h_splits))
    print("    download of match and ignore alone (%.1f MB): " % ((m[0].numel() * 3) / 1e6) + "  ".join("%.4f s" % t for t in downloads))
    if with_host:
        print("(c) evaluate_bbox (host):            " + "  ".join("%.3f s" % t for t in host))
        print("    slowest (b) %.3f s vs fastest (c) %.3f s: %.1fx; stats equal, AP %.6f" % (max(dev), min(host), min(host) / max(dev), out[0][0]))
    else:
        print("    (c) not timed at this size; AP %.6f" % out[0][0])
    sys.stdout.flush()
