"""mbx_loss_fwd_bwd_quality (the IoU as the positives' confidence target: quality focal loss and varifocal loss) against
mbx_loss_fwd_bwd_loc of the same build with the same arguments -- loc_type l2 and giou, gamma = 2, the same weights, without
mining and with neg_per_pos = 3 -- at the two shapes of tools/loss_bench.py (64 images, P = 646, G = 13 and P = 3199,
G = 100): what the float64 positive term (an IoU and two logs for the few lanes that hold a positive; gamma = 2 is a square,
every other gamma >= 1 a pow) costs on top of the focal loss with that location term.

The method is tools/loss_bench.py's: both launches of each call, CALLS calls of each entry captured into a graph of its own,
the graphs warmed up, then replayed alternately for ROUNDS rounds, each replay between a pair of device events; the median
time per call and its range over the rounds, and the ratio of the medians to the partner's.  The boxes are the random ones of
that tool: most pairs are disjoint (q == 0), which runs the same instructions as any other q.  No target was set for the
cost.  What either loss does to AP is not measured: that needs a dataset.
usage: python tools/loss_quality_bench.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, ROUNDS, NEG_PER_POS = 2000, 15, 3
GAMMA, W_POS, W_NEG = 2.0, 1.0, 0.75
LOC = (("l2", 0), ("giou", 2))                               # MBX_LOC_*
MODES = (("loc", 0), ("qfl", 1), ("vfl", 2))                 # the partner (mbx_loss_fwd_bwd_loc), MBX_QUALITY_QFL, MBX_QUALITY_VFL

if __name__ == "__main__":
    import numpy as np, torch
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    l = _lib.lib()
    for B, P, G in ((64, 646, 13), (64, 3199, 100)):
        rng = np.random.RandomState(P)
        n_pos = rng.randint(1, G + 1, B)
        n_pos[0], n_pos[1] = G, 0
        match = -np.ones((B, P), np.int32)
        for b in range(B):
            match[b, rng.permutation(P)[:n_pos[b]]] = rng.permutation(G)[:n_pos[b]]
        match = torch.from_numpy(match).cuda()
        dec = torch.from_numpy(rng.uniform(0, 1, (B, P, 4)).astype(np.float32)).cuda()
        logits = torch.from_numpy((rng.randn(B, P) * 2 - 2).astype(np.float32)).cuda()
        gt = torch.from_numpy(rng.uniform(0, 1, (B, G, 4)).astype(np.float32)).cuda()
        f = dict(dtype=torch.float32, device="cuda")
        loss2, dl, dz = torch.zeros(2, **f), torch.zeros(B, P, 4, **f), torch.zeros(B, P, **f)
        n_neg = torch.zeros(B, dtype=torch.int32, device="cuda")
        q_stats = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
        ws = torch.empty(max(l.mbx_loss_loc_workspace_bytes(B, P), l.mbx_loss_quality_workspace_bytes(B, P)), dtype=torch.uint8,
                         device="cuda")
        head = (dec.data_ptr(), logits.data_ptr(), 1, gt.data_ptr(), match.data_ptr(), 1000.0, 1.0, B, P, G, loss2.data_ptr(),
                dl.data_ptr(), dz.data_ptr())
        tail = (ws.data_ptr(), ws.numel())

        def call(loc_type, quality, neg_per_pos):
            s = torch.cuda.current_stream().cuda_stream
            if quality == 0:
                _lib.check(l.mbx_loss_fwd_bwd_loc(*head, loc_type, 0.0, GAMMA, W_POS, W_NEG, neg_per_pos, 0, n_neg.data_ptr(),
                                                  *tail, s), "mbx_loss_fwd_bwd_loc")
            else:
                _lib.check(l.mbx_loss_fwd_bwd_quality(*head, loc_type, 0.0, quality, GAMMA, W_POS, W_NEG, neg_per_pos, 0,
                                                      n_neg.data_ptr(), q_stats.data_ptr(), *tail, s), "mbx_loss_fwd_bwd_quality")
        entries = [((loc, mode, npp), lambda t=t, q=q, npp=npp: call(t, q, npp))
                   for npp in (0, NEG_PER_POS) for loc, t in LOC for mode, q in MODES]
        graphs = {}
        for name, fn in entries:
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
        mean_q = (q_stats[:, 0].sum() / q_stats[:, 1].sum()).item()
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
        for npp in (0, NEG_PER_POS):
            print("B=%d P=%d G=%d neg_per_pos=%d (%.1f positives per image, mean q %.3f; gamma = %g, weights (%g, %g)): " % (
                      B, P, G, npp, n_pos.mean(), mean_q, GAMMA, W_POS, W_NEG)
                  + "  ".join("%s %s %.2f us (%.2f..%.2f)%s" % (
                      loc, mode, med[(loc, mode, npp)], min(times[(loc, mode, npp)]), max(times[(loc, mode, npp)]),
                      "" if mode == "loc" else " = %.2f x loc" % (med[(loc, mode, npp)] / med[(loc, "loc", npp)]))
                      for loc, _ in LOC for mode, _ in MODES)
                  + "  [median of %d graph replays of %d calls each, alternating]" % (ROUNDS, CALLS), flush=True)
