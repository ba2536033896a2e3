"""mbx_merge_detections_wbf (weighted boxes fusion, avg, IoU 0.55, min_score 0, expected views 1) against
mbx_merge_detections and linear mbx_merge_detections_soft (min_score 0.001) of the same build, on the seeded candidates of
tools/merge_bench.py: (a) 256 images of the config.yaml.example VGA plan (44 rows per image: 1 x 200 + 43 x 50 = 2 350
candidates, k_max 200, max_det 100, IoU 0.5) and (b) 64 images x 80 rows x 200 = 16 000 candidates (max_det 300, IoU 0.3).

The three forms run in one process on the same inputs.  CALLS calls of each are captured into a graph of their own (every
call rewrites all its outputs, so every call does the full work), the graphs are warmed up, then replayed alternately for
ROUNDS rounds, each replay between a pair of device events.  CALLS and ROUNDS are sized to the slower shape, where one fusion
launch is a walk of 16 000 sequential steps.  Reported: the median time per call and its range over the rounds, the ratio to
the plain merge, and the clusters per image.  What fusion does to AP is not measured: that needs a trained model and a
dataset.
usage: python tools/merge_wbf_bench.py [output file]   (default profiles/merge_wbf_bench.txt)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, ROUNDS, WBF_IOU = 5, 9, 0.55

if __name__ == "__main__":
    import numpy as np, torch
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    from multibox_amd.synth import merge_candidates
    l = _lib.lib()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merge_wbf_bench.txt")
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    print(lines[0], flush=True)
    for name, I, rows, K, n_obj, max_det, thr in (("a: VGA plan", 256, 44, 200, 8, 100, 0.5), ("b: 80 full rows", 64, 80, 200, 40, 300, 0.3)):
        count = np.full((I, rows), 200, np.int32)
        if rows == 44:
            count[:, 1:] = 50
        boxes, scores, count, image_rows = merge_candidates(seed=rows, I=I, rows_per_image=(rows, rows), K=K, n_obj=n_obj,
                                                            count=count.reshape(-1))
        R = len(count)
        d_b, d_s, d_c, d_r = (torch.from_numpy(a).cuda() for a in (boxes, scores, count, image_rows))
        o_b = torch.empty((I, max_det, 4), dtype=torch.float64, device="cuda")
        o_s = torch.empty((I, max_det), dtype=torch.float32, device="cuda")
        o_i, o_v = (torch.empty((I, max_det), dtype=torch.int32, device="cuda") for _ in range(2))
        o_c, o_st = (torch.empty((I,), dtype=torch.int32, device="cuda") for _ in range(2))
        ws = torch.empty((l.mbx_merge_wbf_workspace(R, K),), dtype=torch.uint8, device="cuda")
        stream = lambda: torch.cuda.current_stream().cuda_stream
        common = (d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr())
        outs = (o_b.data_ptr(), o_s.data_ptr(), o_i.data_ptr(), o_c.data_ptr(), o_st.data_ptr())

        def plain():
            _lib.check(l.mbx_merge_detections(*common, I, K, max_det, thr, *outs, stream()), "mbx_merge_detections")

        def soft():
            _lib.check(l.mbx_merge_detections_soft(*common, I, K, max_det, 1, thr, 0.5, 0.001, 0.0, *outs, None, stream()),
                       "mbx_merge_detections_soft")

        def wbf():
            _lib.check(l.mbx_merge_detections_wbf(*common, R, I, K, max_det, 1, WBF_IOU, 0.0, 1, *outs, o_v.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), stream()), "mbx_merge_detections_wbf")
        forms = (("merge", plain), ("soft linear", soft), ("wbf avg", wbf))
        graphs, kept = {}, {}
        for form, fn in forms:
            fn()                                               # lazy code-object load, outside the capture
            torch.cuda.synchronize()
            assert int(o_st.max()) == 0
            kept[form] = "%d..%d" % (int(o_c.min()), int(o_c.max()))
            graphs[form] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[form]):
                for _ in range(CALLS):
                    fn()
        # the clusters per image: everything that comes out when max_det does not cut (640 is the entry's limit)
        big = [torch.empty((I, 640) + tail, dtype=dt, device="cuda") for tail, dt in (((4,), torch.float64), ((), torch.float32),
                                                                                      ((), torch.int32), ((), torch.int32))]
        _lib.check(l.mbx_merge_detections_wbf(*common, R, I, K, 640, 1, WBF_IOU, 0.0, 1, big[0].data_ptr(), big[1].data_ptr(),
                                              big[2].data_ptr(), o_c.data_ptr(), o_st.data_ptr(), big[3].data_ptr(), ws.data_ptr(),
                                              ws.numel(), stream()), "mbx_merge_detections_wbf")
        torch.cuda.synchronize()
        clusters, members = o_c.cpu().numpy(), big[3].cpu().numpy()
        for _ in range(2):
            for gr in graphs.values():
                gr.replay()
        torch.cuda.synchronize()
        times = {form: [] for form in graphs}
        for _ in range(ROUNDS):
            for form, gr in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gr.replay()
                b.record()
                torch.cuda.synchronize()
                times[form].append(a.elapsed_time(b) / CALLS * 1e3)
        med = {form: float(np.median(t)) for form, t in times.items()}
        n_cand = int(count.sum()) // I
        lines.append("%s: I=%d candidates per image %d k_max=%d max_det=%d: " % (name, I, n_cand, K, max_det)
                     + "  ".join("%s %.1f us (%.1f..%.1f) %.2f x merge, out %s" % (form, med[form], min(t), max(t), med[form] / med["merge"],
                                                                                 kept[form]) for form, t in times.items())
                     + "  wbf clusters per image at max_det 640: %d..%d (640 = cut), largest cluster %d members"
                       "  [median of %d graph replays of %d calls each, alternating]" % (
                         int(clusters.min()), int(clusters.max()), int(members.max()), ROUNDS, CALLS))
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
