"""mbx_match alone against mbx_match + mbx_match_extend (threshold matching, IoU 0.5) at the headline shape (64 images,
P = 646, G = 13) and the 512x512 shape (P = 3199, G = 100): what the extra launch adds to the matching it follows.

The priors are the real ones of the two configurations; the boxes are jittered copies of random priors, so that a realistic
share of the priors clears the threshold; the predictions are the priors plus noise.  Both forms run in one process on the
same buffers.  CALLS calls of each are captured into a graph of their own (mbx_match rewrites the whole of `match`, so
every call of the pair does the full work), both graphs are warmed up, then replayed alternately for ROUNDS rounds, each
replay between a pair of device events.  Reported: the median time per call and its range over the rounds, and the
difference of the medians -- the microseconds the key adds to a training step.  What threshold matching does to AP is not
measured: that needs a dataset.
usage: python tools/match_extend_bench.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, ROUNDS, THRESHOLD = 200, 15, 0.5

if __name__ == "__main__":
    import numpy as np, torch
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib, priors as PR
    l = _lib.lib()
    for B, G, size, ars in ((64, 13, 299, [1, 2, 3, 1 / 2., 1 / 3.]), (64, 100, 512, [1, 2, 3, 4, 1 / 2., 1 / 3., 1 / 4.])):
        pri = PR.priors_for_input_size(ars, size).astype(np.float32)
        P = pri.shape[0]
        rng = np.random.RandomState(P)
        n = rng.randint(1, G + 1, B).astype(np.int32)
        n[0] = G
        gt = np.zeros((B, G, 4), np.float32)
        for b in range(B):
            gt[b, :n[b]] = pri[rng.randint(0, P, n[b])] + rng.uniform(-0.02, 0.02, (n[b], 4)).astype(np.float32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        priors, gt_d, n_d = dev(pri), dev(gt), dev(n)
        dec = dev((pri[None] + rng.randn(B, P, 4) * 0.05).astype(np.float32))
        conf = dev(rng.uniform(0.01, 0.99, (B, P)).astype(np.float32))
        match = torch.zeros((B, P), dtype=torch.int32, device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        n_extra = torch.zeros((B,), dtype=torch.int32, device="cuda")

        def plain():
            _lib.check(l.mbx_match(dec.data_ptr(), conf.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(), 1000.0, B, P, G,
                                   match.data_ptr(), status.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream),
                       "mbx_match")

        def extended():
            plain()
            _lib.check(l.mbx_match_extend(priors.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(), status.data_ptr(), THRESHOLD,
                                          B, P, G, match.data_ptr(), n_extra.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "mbx_match_extend")
        graphs = {}
        for name, fn in (("match", plain), ("match + extend", extended)):
            fn()                                               # lazy code-object load, outside the capture
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(CALLS):
                    fn()
        for _ in range(3):
            for gr in graphs.values():
                gr.replay()
        graphs["match + extend"].replay()
        torch.cuda.synchronize()
        assert int(status.max()) == 0
        added = n_extra.float().mean().item()
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
        print("B=%d P=%d G=%d iou_threshold=%.2f (%.1f boxes, %.1f priors added per image): " % (B, P, G, THRESHOLD, n.mean(), added)
              + "  ".join("%s %.2f us (%.2f..%.2f)" % (name, med[name], min(t), max(t)) for name, t in times.items())
              + "  added by the extend launch = %.2f us  [median of %d graph replays of %d calls each, alternating]" % (
                  med["match + extend"] - med["match"], ROUNDS, CALLS), flush=True)
