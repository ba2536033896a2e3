"""The ignore band against its partners, at the headline shape (64 images, P = 646, G = 13) and the 512x512 shape (P = 3199,
G = 100), from one build, on the same inputs, in one process.

  * mbx_match_ignore against the mbx_match_extend launch alone, threshold 0.5 then 0.4.  Both update `match` in place and a
    second call on their own output has less to do, so every call is preceded by a device copy of the bipartite match into
    `match`; the copy alone is a third graph and its median is taken off both.  The kernel walks the pairs mbx_match_extend
    walks, without the argmax, and may stop at the first hit: the bar is 1.2 x the partner.
  * mbx_loss_fwd_bwd_ignore against mbx_loss_fwd_bwd_quality (QFL, GIoU) with the same arguments and the same `match` without
    a -2, unmined and mined (3 negatives per positive); the ignore entry on the banded match (threshold matching at 0.5, the
    band at 0.4) is printed beside them.  The flag costs a compare per prior and a count: the bar is 1.1 x the partner.

The priors are the real ones of the two configurations; the boxes are jittered copies of random priors; the predictions are
the priors plus noise (tools/match_extend_bench.py's inputs).  CALLS calls of each form are captured into a graph of its own,
all graphs are warmed up, then replayed alternately for ROUNDS rounds, each replay between a pair of device events.  Reported:
the median time per call and its range over the rounds.  What the band does to AP is not measured: that needs a dataset.
usage: python tools/match_ignore_bench.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, ROUNDS = 200, 15


def alternate(torch, np, forms):
    """{name: fn} -> {name: [microseconds per call, one per round]}: a graph of CALLS calls per form, replayed alternately."""
    graphs = {}
    for name, fn in forms.items():
        fn()                                                   # lazy code-object load, outside the capture
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(CALLS):
                fn()
    for _ in range(3):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):
        for name, gr in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / CALLS * 1e3)
    return times


if __name__ == "__main__":
    import numpy as np, torch
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib, priors as PR
    l = _lib.lib()
    tail = "[median of %d graph replays of %d calls each, alternating]" % (ROUNDS, CALLS)
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
        logits = dev((rng.randn(B, P) * 2 - 2).astype(np.float32))
        conf = dev(rng.uniform(0.01, 0.99, (B, P)).astype(np.float32))
        match = torch.zeros((B, P), dtype=torch.int32, device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        count = torch.zeros((B,), dtype=torch.int32, device="cuda")
        stream = lambda: torch.cuda.current_stream().cuda_stream
        _lib.check(l.mbx_match(dec.data_ptr(), conf.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(), 1000.0, B, P, G,
                               match.data_ptr(), status.data_ptr(), None, 0, stream()), "mbx_match")
        torch.cuda.synchronize()
        assert int(status.max()) == 0
        bipartite = match.clone()

        # ---- the match kernel against the extend launch
        for thr in (0.5, 0.4):
            def copy():
                match.copy_(bipartite)

            def extend():
                copy()
                _lib.check(l.mbx_match_extend(priors.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(), status.data_ptr(), thr, B, P,
                                              G, match.data_ptr(), count.data_ptr(), stream()), "mbx_match_extend")

            def ignore():
                copy()
                _lib.check(l.mbx_match_ignore(priors.data_ptr(), 0, gt_d.data_ptr(), n_d.data_ptr(), status.data_ptr(), thr, B,
                                              P, G, match.data_ptr(), count.data_ptr(), stream()), "mbx_match_ignore")
            times = alternate(torch, np, {"copy": copy, "copy + extend": extend, "copy + ignore": ignore})
            ignore()
            torch.cuda.synchronize()
            ignored = count.float().mean().item()
            med = {k: float(np.median(t)) for k, t in times.items()}
            e, i = med["copy + extend"] - med["copy"], med["copy + ignore"] - med["copy"]
            print("B=%d P=%d G=%d threshold=%.2f (%.1f boxes, %.1f priors ignored per image): " % (B, P, G, thr, n.mean(), ignored)
                  + "  ".join("%s %.2f us (%.2f..%.2f)" % (k, med[k], min(t), max(t)) for k, t in times.items())
                  + "  extend alone = %.2f us  ignore alone = %.2f us  ratio %.3f (bar 1.2)  %s" % (e, i, i / e, tail), flush=True)

        # ---- the loss entry against the quality entry
        match.copy_(bipartite)
        _lib.check(l.mbx_match_extend(priors.data_ptr(), gt_d.data_ptr(), n_d.data_ptr(), status.data_ptr(), 0.5, B, P, G,
                                      match.data_ptr(), count.data_ptr(), stream()), "mbx_match_extend")
        extended = match.clone()
        _lib.check(l.mbx_match_ignore(priors.data_ptr(), 0, gt_d.data_ptr(), n_d.data_ptr(), status.data_ptr(), 0.4, B, P, G,
                                      match.data_ptr(), count.data_ptr(), stream()), "mbx_match_ignore")
        banded = match.clone()
        torch.cuda.synchronize()
        assert not bool((extended == -2).any()) and bool((banded == -2).any())
        f = dict(dtype=torch.float32, device="cuda")
        loss2, dl, dz = torch.zeros(2, **f), torch.zeros(B, P, 4, **f), torch.zeros(B, P, **f)
        n_neg = torch.zeros((B,), dtype=torch.int32, device="cuda")
        qs = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        ws = torch.empty((l.mbx_loss_ignore_workspace_bytes(B, P),), dtype=torch.uint8, device="cuda")
        assert ws.numel() >= l.mbx_loss_quality_workspace_bytes(B, P)

        def loss(entry, m, neg_per_pos):
            def fn():
                _lib.check(getattr(l, entry)(dec.data_ptr(), logits.data_ptr(), 1, gt_d.data_ptr(), m.data_ptr(), 1000.0, 1.0, B,
                                             P, G, loss2.data_ptr(), dl.data_ptr(), dz.data_ptr(), 2, 0.0, 1, 2.0, 1.0, 1.0,
                                             neg_per_pos, 0, n_neg.data_ptr(), qs.data_ptr(), ws.data_ptr(), ws.numel(), stream()),
                           entry)
            return fn
        for neg_per_pos in (0, 3):
            times = alternate(torch, np, {"quality": loss("mbx_loss_fwd_bwd_quality", extended, neg_per_pos),
                                          "ignore": loss("mbx_loss_fwd_bwd_ignore", extended, neg_per_pos),
                                          "ignore, banded match": loss("mbx_loss_fwd_bwd_ignore", banded, neg_per_pos)})
            med = {k: float(np.median(t)) for k, t in times.items()}
            print("B=%d P=%d G=%d loss qfl giou neg_per_pos=%d (%.1f of %d priors a -2 in the banded match): " % (
                B, P, G, neg_per_pos, (banded == -2).sum(1).float().mean().item(), P)
                + "  ".join("%s %.2f us (%.2f..%.2f)" % (k, med[k], min(t), max(t)) for k, t in times.items())
                + "  ratio ignore / quality %.3f (bar 1.1)  %s" % (med["ignore"] / med["quality"], tail), flush=True)
