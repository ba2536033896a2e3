"""mbx_match alone against mbx_match + mbx_match_extend (threshold matching, IoU 0.5), mbx_match + mbx_match_atss (ATSS, topk 9)
and mbx_match + mbx_match_tal (task-aligned matching, topk 13, alpha 1, beta 6) at the headline shape (64 images, P = 646,
G = 13) and the 512x512 shape (P = 3199, G = 100): what each extra launch adds to the matching it follows.

The priors and their pyramid levels are the real ones of the two configurations; the boxes are jittered copies of random
priors; the predictions are the priors plus a small jitter (uniform, +-0.02), the scores uniform in (0.01, 0.99).  The four
forms run in one process on the same buffers.  CALLS calls of each are captured into a graph of their own (mbx_match rewrites
the whole of `match`, so every call does the full work), the graphs are warmed up, then replayed alternately for ROUNDS
rounds, each replay between a pair of device events.  Reported: the median time per call and its range over the rounds, the
difference to mbx_match alone, and the priors each rule adds per image.  What any rule does to AP is not measured: that
needs a dataset.
usage: python tools/match_tal_bench.py [output file]   (default profiles/match_tal_bench.txt)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS, ROUNDS, THRESHOLD, ATSS_TOPK, TAL_TOPK, TAL_HALVES, TAL_BETA = 200, 15, 0.5, 9, 13, 2, 6

if __name__ == "__main__":
    import ctypes
    import numpy as np, torch
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib, priors as PR
    l = _lib.lib()
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "match_tal_bench.txt")
    lines = ["device: %s" % torch.cuda.get_device_name(0)]
    print(lines[0], flush=True)
    for B, G, size, ars in ((64, 13, 299, [1, 2, 3, 1 / 2., 1 / 3.]), (64, 100, 512, [1, 2, 3, 4, 1 / 2., 1 / 3., 1 / 4.])):
        pri = PR.priors_for_input_size(ars, size).astype(np.float32)
        P = pri.shape[0]
        grids, last = PR.head_grids(size)
        levels = np.concatenate([[0], np.cumsum([gr * gr * len(ars) for gr in grids] + [last])]).tolist()
        assert levels[-1] == P
        table = (ctypes.c_int32 * len(levels))(*levels)
        rng = np.random.RandomState(P)
        n = rng.randint(1, G + 1, B).astype(np.int32)
        n[0] = G
        gt = np.zeros((B, G, 4), np.float32)
        for b in range(B):
            gt[b, :n[b]] = pri[rng.randint(0, P, n[b])] + rng.uniform(-0.02, 0.02, (n[b], 4)).astype(np.float32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        priors, gt_d, n_d = dev(pri), dev(gt), dev(n)
        dec = dev((pri[None] + rng.uniform(-0.02, 0.02, (B, P, 4))).astype(np.float32))
        conf = dev(rng.uniform(0.01, 0.99, (B, P)).astype(np.float32))
        match = torch.zeros((B, P), dtype=torch.int32, device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        counts = {name: torch.zeros((B,), dtype=torch.int32, device="cuda") for name in ("extend", "atss", "tal")}
        thr = torch.zeros((B, G), dtype=torch.float64, device="cuda")
        stream = lambda: torch.cuda.current_stream().cuda_stream

        def plain():
            _lib.check(l.mbx_match(dec.data_ptr(), conf.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(), 1000.0, B, P, G,
                                   match.data_ptr(), status.data_ptr(), None, 0, stream()), "mbx_match")

        def extended():
            plain()
            _lib.check(l.mbx_match_extend(priors.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(), status.data_ptr(), THRESHOLD,
                                          B, P, G, match.data_ptr(), counts["extend"].data_ptr(), stream()), "mbx_match_extend")

        def atss():
            plain()
            _lib.check(l.mbx_match_atss(priors.data_ptr(), table, len(levels) - 1, gt_d.data_ptr(), n_d.data_ptr(),
                                        status.data_ptr(), ATSS_TOPK, B, P, G, match.data_ptr(), counts["atss"].data_ptr(),
                                        thr.data_ptr(), stream()), "mbx_match_atss")

        def tal():
            plain()
            _lib.check(l.mbx_match_tal(priors.data_ptr(), dec.data_ptr(), conf.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(),
                                       status.data_ptr(), TAL_TOPK, TAL_HALVES, TAL_BETA, B, P, G, match.data_ptr(),
                                       counts["tal"].data_ptr(), thr.data_ptr(), stream()), "mbx_match_tal")
        forms = (("match", plain), ("match + extend", extended), ("match + atss", atss), ("match + tal", tal))
        graphs = {}
        for name, fn in forms:
            fn()                                               # lazy code-object load, outside the capture
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(CALLS):
                    fn()
        for _ in range(3):
            for gr in graphs.values():
                gr.replay()
        torch.cuda.synchronize()
        assert int(status.max()) == 0
        added = {name: counts[name].float().mean().item() for name in counts}
        times = {name: [] for name in graphs}
        for _ in range(ROUNDS):
            for name, gr in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gr.replay()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) / CALLS * 1e3)
        med = {name: float(np.median(t)) for name, t in times.items()}
        lines.append("B=%d P=%d G=%d (%.1f boxes per image): " % (B, P, G, n.mean())
                     + "  ".join("%s %.2f us (%.2f..%.2f)" % (name, med[name], min(t), max(t)) for name, t in times.items())
                     + "  extend at %.2f adds %.2f us and %.1f priors per image, atss at topk %d adds %.2f us and %.1f priors per"
                       " image, tal at topk %d, alpha %.1f, beta %d adds %.2f us and %.1f priors per image"
                       "  [median of %d graph replays of %d calls each, alternating]" % (
                         THRESHOLD, med["match + extend"] - med["match"], added["extend"], ATSS_TOPK,
                         med["match + atss"] - med["match"], added["atss"], TAL_TOPK, TAL_HALVES / 2.0, TAL_BETA,
                         med["match + tal"] - med["match"], added["tal"], ROUNDS, CALLS))
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
