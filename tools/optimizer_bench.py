"""What the optimiser choice costs, at the full network's parameter counts (nW filters, nBt betas: Net at 299 x 299, k = 5).

Five groups of launches on buffers of the same sizes in one process, each over the filters (L2 coefficient WEIGHT_DECAY, the
bf16 copy refreshed, reg_loss added to) and then the betas, as the trainer calls them:
  rmsprop       mbx_rmsprop_ema_step, momentum 0 -- the partner: 30 bytes per filter (w, g, ms, ema read; w, ms, ema written;
                the bf16 copy written), 28 per beta;
  sgd           mbx_sgd_ema_step, momentum 0.9: the accumulator in the place of ms -- the same 30 and 28 bytes;
  adam          mbx_adam_ema_step: two moments -- 38 bytes per filter, 36 per beta;
  sgd_clipped,  the clipped instantiations of the two, with a clip block of scale 1: the same bytes as the plain ones.
  adam_clipped
CALLS calls of each are captured into a graph of their own, the graphs are warmed up, then replayed alternately for ROUNDS
rounds, each replay between a pair of device events.  Reported: the median time per call with its range, the bytes the
algorithm needs over that time, and each rule's bytes/s over rmsprop's of the same replays (the rules run the same loop over
the same kind of streams, so each should reach 0.9 of it).

What the rules do to AP or convergence on real data is not measured: that needs a dataset.
usage: python tools/optimizer_bench.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, ROUNDS = 20, 15
BAR = 0.9


def kernels():
    import numpy as np, torch
    from multibox_amd import _lib
    from multibox_amd.engine import Net, WEIGHT_DECAY
    l = _lib.lib()
    net = Net(batch=2, input_size=299, k=5, mode="train", seed=2)
    nW, nBt = net.nW, net.nBt
    del net
    torch.cuda.empty_cache()
    f = dict(dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    bufs = {}
    for name, n in (("W", nW), ("Bt", nBt)):
        w = torch.randn(n, generator=gen, **f) * 0.05
        bufs[name] = dict(n=n, w=w, g=torch.randn(n, generator=gen, **f) * 0.01, ms=torch.ones(n, **f), m=torch.zeros(n, **f),
                          v=torch.zeros(n, **f), ema=w.clone(), wb=torch.zeros(n, dtype=torch.bfloat16, device="cuda") if name == "W" else None)
    ctl, clip = torch.zeros(8, **f), torch.zeros(8, **f)
    clip[2] = 1.0
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    reg = torch.zeros(1, **f)
    S = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    ranges = lambda: ((bufs["W"], WEIGHT_DECAY, reg.data_ptr()), (bufs["Bt"], 0.0, None))

    def rmsprop():
        for b, wd, r in ranges():
            _lib.check(l.mbx_rmsprop_ema_step(p(b["w"]), p(b["g"]), p(b["ms"]), None, p(b["ema"]), p(b["wb"]), b["n"], 0.01, 0.9, 0.0, 1.0, wd,
                                              0.9999, 1, r, ctl.data_ptr(), S()), "rmsprop")

    def sgd(gate, clipped):
        for b, wd, r in ranges():
            _lib.check(l.mbx_sgd_ema_step(p(b["w"]), p(b["g"]), p(b["m"]), p(b["ema"]), p(b["wb"]), b["n"], 0.01, 0.9, 0, wd, 0.9999, 1, r,
                                          gate.data_ptr(), clipped, S()), "sgd")

    def adam(gate, clipped):
        for b, wd, r in ranges():
            _lib.check(l.mbx_adam_ema_step(p(b["w"]), p(b["g"]), p(b["m"]), p(b["v"]), p(b["ema"]), p(b["wb"]), b["n"], 0.001, 0.9, 0.999, 1e-8,
                                           wd, 0.0, 1000, skipped.data_ptr(), 0.9999, 1, r, gate.data_ptr(), clipped, S()), "adam")

    entries = [("rmsprop", rmsprop), ("sgd", lambda: sgd(ctl, 0)), ("adam", lambda: adam(ctl, 0)),
               ("sgd_clipped", lambda: sgd(clip, 1)), ("adam_clipped", lambda: adam(clip, 1))]
    per = {"rmsprop": (30, 28), "sgd": (30, 28), "adam": (38, 36), "sgd_clipped": (30, 28), "adam_clipped": (38, 36)}
    nbytes = {name: fw * nW + fb * nBt for name, (fw, fb) in per.items()}
    graphs = {}
    for name, fn in entries:
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
    for b in bufs.values():
        assert bool(torch.isfinite(b["w"]).all()), "the weights left the finite range"
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
    rate = {name: nbytes[name] / (med[name] * 1e-6) for name in med}
    print("nW=%d nBt=%d  [median of %d graph replays of %d calls each, alternating; a call = filters + betas]" % (nW, nBt, ROUNDS, CALLS))
    for name, t in times.items():
        print("  %-13s %7.1f us (%.1f..%.1f)  %7.1f MB  %.2f TB/s  bytes/s over rmsprop's %.3f%s" % (
            name, med[name], min(t), max(t), nbytes[name] / 1e6, rate[name] / 1e12, rate[name] / rate["rmsprop"],
            "" if name == "rmsprop" else "  (bar %.1f: %s)" % (BAR, "met" if rate[name] >= BAR * rate["rmsprop"] else "MISSED")), flush=True)


if __name__ == "__main__":
    import __graft_entry__ as g
    g.build()
    kernels()
