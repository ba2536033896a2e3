"""What LAYERWISE_TRUST costs, at the full network's trainable filter range (nW filters: Net at 299 x 299, k = 5) with the real
partition of net.param_index (the plan the Trainer builds).

Groups of launches on buffers of that size in one process, each beside its partner of the same build:
  sqnorm        mbx_grad_sqnorm over the range (g and w, wd = WEIGHT_DECAY) -- the partner of the norm pass: 8 bytes per filter;
  norms_sgd     mbx_trust_norms_sgd: the same 8 bytes, two sums per chunk (bar: 0.8 of sqnorm's bytes/s);
  sgd           mbx_sgd_ema_step, momentum 0.9 -- the partner of the LARS apply pass: 30 bytes per filter;
  sgd_trust     mbx_sgd_ema_step_trust: the same 30 bytes (bar: 0.9 of sgd's bytes/s);
  adam          mbx_adam_ema_step -- the partner of LAMB's two passes: 38 bytes per filter;
  lamb_passes   mbx_trust_moments_adam (w, g, m, v read; m, v written: 24 bytes) + mbx_adam_ema_step_trust (w, m, v, ema read; w,
                ema written; the bf16 copy: 26 bytes) = 50 bytes, both passes' bytes over the sum of their time (bar: 0.9 of adam's);
  ratios        mbx_trust_ratios alone;
  lars, lamb    the whole range step under the key: norm pass + ratios + apply pass; less sgd / adam = the added time per step.
CALLS calls of each are captured into a graph of their own, the graphs are warmed up, then replayed alternately for ROUNDS
rounds, each replay between a pair of device events.  Reported: the median time per call with its range, the bytes the
algorithm needs over that time and the ratio to the partner's bytes/s in the same replays.

The training step under the new keys is not timed, and what LARS / LAMB do to AP or convergence on real data is not measured:
that needs a dataset.
usage: python tools/trust_bench.py [--out profiles/trust_bench.txt]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS, ROUNDS = 20, 15


def kernels(say):
    import ctypes as C
    import numpy as np, torch
    from multibox_amd import _lib
    from multibox_amd.engine import Net, WEIGHT_DECAY
    l = _lib.lib()
    net = Net(batch=2, input_size=299, k=5, mode="train", seed=2)
    nW = net.nW
    ents = sorted((off, len(shape) > 1) for name, (buf, off, shape, _) in net.param_index.items() if buf == "W")
    del net
    torch.cuda.empty_cache()
    nv = len(ents)
    bounds = (C.c_int64 * (nv + 1))(*([0] + [off for off, _ in ents[1:]] + [nW]))
    adapt = (C.c_int32 * nv)(*[int(a) for _, a in ents])
    nc = int(l.mbx_trust_plan_count(bounds, nv))
    chunks_h, vars_h = (_lib.TrustChunk * nc)(), (_lib.TrustVar * nv)()
    _lib.check(l.mbx_trust_plan(bounds, adapt, nv, chunks_h, vars_h), "plan")
    up = lambda a: torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda()
    chunks, vars_ = up(chunks_h), up(vars_h)
    CH = int(l.mbx_trust_chunk_elems())
    f = dict(dtype=torch.float32, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn(nW, generator=gen, **f) * 0.05
    b = dict(w=w, g=torch.randn(nW, generator=gen, **f) * 0.01, m=torch.zeros(nW, **f), v=torch.zeros(nW, **f), ema=w.clone(),
             wb=torch.zeros(nW, dtype=torch.bfloat16, device="cuda"))
    part = torch.zeros(2 * nc, dtype=torch.float64, device="cuda")
    sq_part = torch.zeros(int(l.mbx_grad_sqnorm_partials(nW)), dtype=torch.float64, device="cuda")
    ratio = torch.ones(nv, **f)
    ctl = torch.zeros(8, **f)
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    reg = torch.zeros(1, **f)
    S = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    wd = WEIGHT_DECAY
    tail = lambda: (p(chunks), nc, p(ratio), S())

    def sqnorm():
        _lib.check(l.mbx_grad_sqnorm(p(b["g"]), p(b["w"]), nW, wd, p(sq_part), S()), "sqnorm")

    def norms_sgd():
        _lib.check(l.mbx_trust_norms_sgd(p(b["w"]), p(b["g"]), p(chunks), nc, wd, p(part), p(ctl), 0, S()), "norms_sgd")

    def ratios(coeff):
        _lib.check(l.mbx_trust_ratios(p(part), p(vars_), nv, coeff, p(ratio), p(ctl), S()), "ratios")

    def sgd():
        _lib.check(l.mbx_sgd_ema_step(p(b["w"]), p(b["g"]), p(b["m"]), p(b["ema"]), p(b["wb"]), nW, 0.01, 0.9, 0, wd, 0.9999, 1, p(reg),
                                      p(ctl), 0, S()), "sgd")

    def sgd_trust():
        _lib.check(l.mbx_sgd_ema_step_trust(p(b["w"]), p(b["g"]), p(b["m"]), p(b["ema"]), p(b["wb"]), nW, 0.01, 0.9, 0, wd, 0.9999, 1,
                                            p(reg), p(ctl), 0, *tail()), "sgd_trust")

    def adam():
        _lib.check(l.mbx_adam_ema_step(p(b["w"]), p(b["g"]), p(b["m"]), p(b["v"]), p(b["ema"]), p(b["wb"]), nW, 0.001, 0.9, 0.999, 1e-8, wd,
                                       0.0, 1000, p(skipped), 0.9999, 1, p(reg), p(ctl), 0, S()), "adam")

    def moments():
        _lib.check(l.mbx_trust_moments_adam(p(b["w"]), p(b["g"]), p(b["m"]), p(b["v"]), p(chunks), nc, 0.9, 0.999, 1e-8, wd, 0.0, 1000,
                                            p(skipped), p(part), p(ctl), 0, S()), "moments")

    def adam_trust():
        _lib.check(l.mbx_adam_ema_step_trust(p(b["w"]), p(b["g"]), p(b["m"]), p(b["v"]), p(b["ema"]), p(b["wb"]), nW, 0.001, 0.9, 0.999,
                                             1e-8, wd, 0.0, 1000, p(skipped), 0.9999, 1, p(reg), p(ctl), 0, *tail()), "adam_trust")

    def lamb_passes():
        moments()
        adam_trust()

    def lars():
        norms_sgd()
        ratios(0.001)
        sgd_trust()

    def lamb():
        moments()
        ratios(1.0)
        adam_trust()

    entries = [("sqnorm", sqnorm, 8, None), ("norms_sgd", norms_sgd, 8, ("sqnorm", 0.8)), ("sgd", sgd, 30, None),
               ("sgd_trust", sgd_trust, 30, ("sgd", 0.9)), ("adam", adam, 38, None), ("lamb_passes", lamb_passes, 50, ("adam", 0.9)),
               ("ratios", lambda: ratios(0.001), 0, None), ("lars", lars, 38, None), ("lamb", lamb, 50, None)]
    graphs = {}
    for name, fn, _, _ in entries:
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
    assert bool(torch.isfinite(b["w"]).all()), "the weights left the finite range"
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / CALLS * 1e3)
    med = {name: float(np.median(t)) for name, t in times.items()}
    r = ratio.cpu().numpy()[np.array([a for _, a in ents])]
    say("nW=%d  chunk %d elements  %d variables (%d adapt)  %d chunks  [median of %d graph replays of %d calls each, alternating]" % (
        nW, CH, nv, int(sum(a for _, a in ents)), nc, ROUNDS, CALLS))
    for name, _, per, partner in entries:
        t, nb = times[name], per * nW
        line = "  %-12s %7.1f us (%.1f..%.1f)" % (name, med[name], min(t), max(t))
        if per:
            line += "  %7.1f MB  %.2f TB/s" % (nb / 1e6, nb / (med[name] * 1e-6) / 1e12)
        if partner:
            pn, bar = partner
            pper = [e[2] for e in entries if e[0] == pn][0]
            rel = (per / med[name]) / (pper / med[pn])
            line += "  bytes/s over %s's %.3f  (bar %.1f: %s)" % (pn, rel, bar, "met" if rel >= bar else "MISSED")
        say(line)
    say("  added per step: LARS %+.1f us over sgd, LAMB %+.1f us over adam" % (med["lars"] - med["sgd"], med["lamb"] - med["adam"]))
    say("  ratios of the adapting variables after the last call: min %.3g median %.3g max %.3g" % (r.min(), float(np.median(r)), r.max()))


if __name__ == "__main__":
    import __graft_entry__ as g
    g.build()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "trust_bench.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    kernels(say)
    with open(out, "w") as fh:
        fh.write("python tools/trust_bench.py, one process on one MI355X:\n" + "\n".join(lines) + "\n")
