"""mbx_loss_fwd_bwd against mbx_loss_fwd_bwd_mined (hard-negative mining, neg_per_pos = 3) and mbx_loss_fwd_bwd_focal (the
focal loss, gamma = 2, alpha = 0.25, without mining and with neg_per_pos = 3) at the headline shape (64 images, P = 646,
G = 13) and the 512x512 shape (P = 3199, G = 100): what the selection, and the power per prior, cost on top of the loss.

The entry points run in one process on the same buffers.  A call is two launches of a few microseconds, so a host loop
would time the enqueue: CALLS calls of each are captured into a graph of their own, the graphs are warmed up, then
replayed alternately for ROUNDS rounds, each replay between a pair of device events.  Reported: the median time per call
and its range over the rounds, and the ratios of the medians (focal against unmined, focal_mined against mined: the same
selection).  A second line per shape has mbx_loss_fwd_bwd_loc (the choice of location term) once per type -- plain confidence
term, no mining, smooth-L1 at beta = 0.1 -- against the unmined entry: what the float64 term of the few positives and the
larger kernel cost.  The boxes are the random ones of the other rows (an IoU is an IoU of whatever it is given); the time
does not depend on their values beyond the branch a pair takes.  What mining, the focal loss or the location term do to AP
is not measured: that needs a dataset.
usage: python tools/loss_bench.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, ROUNDS, NEG_PER_POS = 2000, 15, 3
FOCAL_GAMMA, FOCAL_ALPHA = 2.0, 0.25
LOC_TYPES, LOC_BETA = ("l2", "smooth_l1", "giou", "diou", "ciou"), 0.1      # MBX_LOC_L2 = 0 .. MBX_LOC_CIOU = 4

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
        ws = torch.empty(max(l.mbx_loss_workspace_bytes(B), l.mbx_loss_mined_workspace_bytes(B, P),
                             l.mbx_loss_focal_workspace_bytes(B, P), l.mbx_loss_loc_workspace_bytes(B, P)),
                         dtype=torch.uint8, device="cuda")
        head = (dec.data_ptr(), logits.data_ptr(), 1, gt.data_ptr(), match.data_ptr(), 1000.0, 1.0, B, P, G, loss2.data_ptr(),
                dl.data_ptr(), dz.data_ptr())
        tail = (ws.data_ptr(), ws.numel())

        def plain():
            _lib.check(l.mbx_loss_fwd_bwd(*head, *tail, torch.cuda.current_stream().cuda_stream), "mbx_loss_fwd_bwd")

        def mined():
            _lib.check(l.mbx_loss_fwd_bwd_mined(*head, NEG_PER_POS, 0, n_neg.data_ptr(), *tail,
                                                torch.cuda.current_stream().cuda_stream), "mbx_loss_fwd_bwd_mined")

        def focal(neg_per_pos=0):
            _lib.check(l.mbx_loss_fwd_bwd_focal(*head, FOCAL_GAMMA, FOCAL_ALPHA, 1.0 - FOCAL_ALPHA, neg_per_pos, 0,
                                                n_neg.data_ptr(), *tail, torch.cuda.current_stream().cuda_stream),
                       "mbx_loss_fwd_bwd_focal")

        def loc(loc_type):
            _lib.check(l.mbx_loss_fwd_bwd_loc(*head, loc_type, LOC_BETA, 0.0, 1.0, 1.0, 0, 0, n_neg.data_ptr(), *tail,
                                              torch.cuda.current_stream().cuda_stream), "mbx_loss_fwd_bwd_loc")
        graphs = {}
        entries = [("unmined", plain), ("mined", mined), ("focal", focal), ("focal_mined", lambda: focal(NEG_PER_POS))]
        entries += [("loc_" + name, lambda t=t: loc(t)) for t, name in enumerate(LOC_TYPES)]
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
        mined()                                                # n_neg as the mined entry leaves it
        torch.cuda.synchronize()
        kept = n_neg.float().mean().item()
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
        print("B=%d P=%d G=%d neg_per_pos=%d (%.1f of %.1f negatives kept per image): " % (B, P, G, NEG_PER_POS, kept, P - n_pos.mean())
              + "  ".join("%s %.2f us (%.2f..%.2f)" % (name, med[name], min(t), max(t)) for name, t in times.items()
                          if not name.startswith("loc_"))
              + "  mined / unmined = %.2f  focal / unmined = %.2f  focal_mined / mined = %.2f  [focal: gamma = %g, alpha = %g; "
                "median of %d graph replays of %d calls each, alternating]" % (
                  med["mined"] / med["unmined"], med["focal"] / med["unmined"], med["focal_mined"] / med["mined"],
                  FOCAL_GAMMA, FOCAL_ALPHA, ROUNDS, CALLS), flush=True)
        print("B=%d P=%d G=%d loc (%.1f positives per image; gamma = 0, weights (1, 1), no mining, beta = %g; same replays): " % (
                  B, P, G, n_pos.mean(), LOC_BETA)
              + "  ".join("%s %.2f us (%.2f..%.2f) = %.2f x unmined" % (name[4:], med[name], min(t), max(t), med[name] / med["unmined"])
                          for name, t in times.items() if name.startswith("loc_")), flush=True)
