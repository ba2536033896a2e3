"""What CLIP_GRADIENT_NORM costs, at the full network's parameter counts (nW filters, nBt betas: Net at 299 x 299, k = 5).

Kernels.  Three groups of launches on the same buffers in one process:
  norm     mbx_grad_sqnorm over the filters (g and w, wd = WEIGHT_DECAY) and over the betas (g alone), then mbx_clip_finalize:
           what the key adds to a step -- 8 bytes read per filter, 4 per beta;
  plain    mbx_rmsprop_ema_step over the filters and the betas, as the trainer calls it (momentum 0): 30 bytes per filter
           (w, g, ms, ema read; ema, ms, w written; the bf16 copy written), 28 per beta;
  clipped  mbx_rmsprop_ema_step_clipped on the same arguments with a clip block of scale 1: the same bytes.
CALLS calls of each are captured into a graph of their own, the graphs are warmed up, then replayed alternately for ROUNDS
rounds, each replay between a pair of device events.  Reported: the median time per call with its range, the bytes the
algorithm needs over that time, and norm's bytes/s over plain's (the norm only reads, so it should stream at least as
fast; 0.8 is the bar: the margin is its double accumulation and the reduction tail).

Step (--step).  Two trainers at the benchmark's shape (batch 64, synthetic batch, captured graphs), one without the key and
one with clip_gradient_norm = inf, warmed up, then PAIRS alternating pairs of STEPS steps each between host clocks that end in
a device synchronise.  Reported: ms per step of each leg of each pair and the difference of the medians.

What clipping does to AP on real data is not measured: that needs a dataset.
usage: python tools/clip_bench.py [--step]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, ROUNDS = 20, 15
PAIRS, STEPS, WARMUP, BATCH = 3, 60, 10, 64


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
        bufs[name] = dict(n=n, w=w, g=torch.randn(n, generator=gen, **f) * 0.01, ms=torch.ones(n, **f), ema=w.clone(),
                          wb=torch.zeros(n, dtype=torch.bfloat16, device="cuda") if name == "W" else None)
    slots = [int(l.mbx_grad_sqnorm_partials(n)) for n in (nW, nBt)]
    part = torch.zeros(sum(slots), dtype=torch.float64, device="cuda")
    ctl, clip = torch.zeros(8, **f), torch.zeros(8, **f)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    reg = torch.zeros(1, **f)
    S = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()

    def norm():
        W, Bt = bufs["W"], bufs["Bt"]
        _lib.check(l.mbx_grad_sqnorm(p(W["g"]), p(W["w"]), nW, WEIGHT_DECAY, part.data_ptr(), S()), "grad_sqnorm W")
        _lib.check(l.mbx_grad_sqnorm(p(Bt["g"]), None, nBt, 0.0, part.data_ptr() + 8 * slots[0], S()), "grad_sqnorm beta")
        _lib.check(l.mbx_clip_finalize(part.data_ptr(), sum(slots), float("inf"), ctl.data_ptr(), clip.data_ptr(), counts.data_ptr(), S()),
                   "clip_finalize")

    def step(entry, gate):
        for name, wd in (("W", WEIGHT_DECAY), ("Bt", 0.0)):
            b = bufs[name]
            _lib.check(entry(p(b["w"]), p(b["g"]), p(b["ms"]), None, p(b["ema"]), p(b["wb"]), b["n"], 0.01, 0.9, 0.0, 1.0, wd, 0.9999, 1,
                             reg.data_ptr() if wd else None, gate.data_ptr(), S()), "rmsprop " + name)

    entries = [("norm", norm), ("plain", lambda: step(l.mbx_rmsprop_ema_step, ctl)),
               ("clipped", lambda: step(l.mbx_rmsprop_ema_step_clipped, clip))]
    nbytes = {"norm": 8 * nW + 4 * nBt, "plain": 30 * nW + 28 * nBt, "clipped": 30 * nW + 28 * nBt}
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
    assert float(clip[2]) == 1.0 and float(clip[1]) == 0.0 and counts.tolist() == [0, 0], (clip.tolist(), counts.tolist())
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
    print("nW=%d nBt=%d (norm: %d + %d slots, grad norm %.6g): " % (nW, nBt, slots[0], slots[1], float(clip[3]))
          + "  ".join("%s %.1f us (%.1f..%.1f) %.1f MB = %.2f TB/s" % (name, med[name], min(t), max(t), nbytes[name] / 1e6, rate[name] / 1e12)
                      for name, t in times.items())
          + "  norm / plain bytes/s = %.2f (bar 0.8)  clipped / plain time = %.3f  [median of %d graph replays of %d calls each, "
            "alternating]" % (rate["norm"] / rate["plain"], med["clipped"] / med["plain"], ROUNDS, CALLS), flush=True)


def whole_step():
    import numpy as np, torch
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer, decay_steps
    from multibox_amd import priors as PR
    from multibox_amd.synth import synthetic_batch, DEFAULT_ASPECT_RATIOS
    priors = PR.priors_for_input_size(DEFAULT_ASPECT_RATIOS[5], 299).astype(np.float32)
    images, gt, n = synthetic_batch(BATCH, 299, 13, seed=0)
    legs = {}
    for name, key in (("off", None), ("inf", float("inf"))):
        net = Net(batch=BATCH, input_size=299, k=5, mode="train", seed=2)
        tr = Trainer(net, priors, max_num_bboxes=13, location_loss_alpha=1000.0, decay_steps_=decay_steps(56945, BATCH, 4),
                     clip_gradient_norm=key)
        tr.set_batch(torch.from_numpy(images).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n).cuda())
        for _ in range(WARMUP):
            tr.step()
        torch.cuda.synchronize()
        legs[name] = tr
    ms = {name: [] for name in legs}
    for _ in range(PAIRS):
        for name, tr in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                tr.step()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / STEPS * 1e3)
    for name, tr in legs.items():
        assert int(tr.skipped_steps) == 0 and int(tr.match_status().max()) == 0, name
    tr = legs["inf"]
    print("training step, batch %d, 299 x 299, graphs, %d alternating pairs of %d steps: " % (BATCH, PAIRS, STEPS)
          + "  ".join("%s %s ms" % (name, " ".join("%.3f" % v for v in t)) for name, t in ms.items())
          + "  median inf - off = %+.3f ms  [inf: grad norm %.4g, scale %g, clipped %d, non-finite %d]" % (
              float(np.median(ms["inf"]) - np.median(ms["off"])), tr.grad_norm(), tr.clip_scale(), tr.clipped_steps(),
              tr.nonfinite_steps()), flush=True)


if __name__ == "__main__":
    import __graft_entry__ as g
    g.build()
    whole_step() if "--step" in sys.argv[1:] else kernels()
