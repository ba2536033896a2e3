#!/usr/bin/env python3
"""Headline benchmark: images/sec of the full Multibox training step (Inception-ResNet-v2 +
heads forward, on-device matching + loss, backward, RMSProp/EMA) on 299x299 synthetic input,
5 aspect-ratio priors (P=646), BATCH_SIZE=64 per GPU, bf16 storage / fp32 accumulate.

  python bench.py --gpus 1 --steps 20 --warmup 5
  python bench.py --gpus N ...          (starts N ranks itself: launch_plan / spawn_ranks below)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (the driver's form)

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps steps and prints the
line (`value`, `ms_per_step`, ...); `--dump-outputs DIR` also writes what one step of the timed path
computes from the seeded starting state (dump_outputs below).  Everything else it measures runs only
under `--full`: `roofline` prices the dominant kernel (the MFMA implicit-GEMM convolution, forward +
data-gradient launches) from the kernels' begin/end timestamps over three extra real steps after the
timed region (ROCm tracer via torch.profiler; HIP-event intervals of one eager pass as a cross-check); `cpu_baseline` times the restated CPU reference
(oracle/cpu_train.py) on a bounded sample on the host cores; `detect`, `input_augment` and `configs`
are the other BASELINE configurations.  The --no-* switches leave parts of a --full run out.

  python bench.py --gpus 1 --steps 20 --warmup 5 --full
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_DENSE_PEAK_TFLOPS = 2500.0     # MI355X_MICROARCH.md: ~2.5 PF dense bf16
HBM_PEAK_GBS = 8000.0


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="BATCH_SIZE per GPU (BASELINE configs[1]: 64)")
    ap.add_argument("--input-size", type=int, default=299)
    ap.add_argument("--k", type=int, default=5, help="aspect ratios per cell")
    ap.add_argument("--max-num-bboxes", type=int, default=13)
    ap.add_argument("--fine-tune", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-detect", action="store_true", help="skip the detect leg (BASELINE config 4)")
    ap.add_argument("--detect-batch", type=int, default=256)
    ap.add_argument("--detect-steps", type=int, default=10)
    ap.add_argument("--log-losses", action="store_true", help="print the loss after every step to stderr (adds host syncs)")
    ap.add_argument("--no-configs", action="store_true", help="skip the other single-GPU BASELINE configurations (fine-tune, 512x512)")
    ap.add_argument("--config-steps", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="also the roofline / kernel trace, CPU baseline, detect and input-augmentation legs and the other configurations")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what one step of the timed path computes from the seeded starting state as DIR/<name>.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


DUMP_MAX_ELEMENTS = 1 << 20      # per array (4 MB of float32): the arrays of dump_outputs stay far below 64 MB


def dump_indices(n, seed=0):
    """Positions of the fixed, seeded sample dump_outputs keeps of a flat array of n elements (None: all of them)."""
    import numpy as np
    if n <= DUMP_MAX_ELEMENTS:
        return None
    return np.unique(np.random.default_rng(seed).integers(0, n, DUMP_MAX_ELEMENTS))


def training_state(tr, net):
    """Every buffer a training step reads and the optimiser rewrites (parameters, their bf16 copy, RMSProp / momentum
    slots, EMA shadows, batch-norm moving statistics); the rest of a step is recomputed from these and the batch."""
    ts = [net.W, net.Wb, net.Bt, net.MM, net.MV, tr.Wms, tr.Btms, tr.Wmom, tr.Btmom, tr.Wema, tr.Btema, tr.MMema, tr.MVema]
    return [t for t in ts if t is not None]


def dump_outputs(path, tr, net, seeded_state, rank=0, pg=None):
    """--dump-outputs: one step of the timed path (Trainer.step, the same captured graphs) from the seeded state the timed
    steps started from, and what it computed, as DIR/<name>.npy: the losses (float64: location, confidence,
    regularization, total), the heads' predictions of its forward pass, the loss gradients it took of them, the
    batch-norm moving statistics it left, and, for the Multibox heads, the weight / beta gradients of its backward pass
    and the parameters the RMSProp update left (float32).  seeded_state = (global_step, copies of training_state())
    from before the warm-up.
    Why one step from the seeded state, and why the heads: outside MBX_DETERMINISTIC mode the one-launch batch-norm
    backward sums its per-channel statistics with float atomics, and the activation gradient it returns is the small
    difference of large terms, so below the first such layer the gradients of one step from the same state differ
    between runs by up to ~10 % (relative L2 per tensor; 2e-7 with the three-launch form), and so do the weights updated
    from them and every later step.  The heads' gradients come from the loss before any such layer: they agree between
    runs to the rounding of their float-atomic sums (measured 2.4e-5 of the largest gradient; 7e-4 of the largest head
    weight after the update).  An array of more than DUMP_MAX_ELEMENTS elements is stored flat as the seeded sample dump_indices()
    picks, so that two builds can be compared output for output.  Every rank takes the step (a data-parallel step
    all-reduces); rank 0 writes."""
    import numpy as np
    import torch
    step0, saved = seeded_state
    for t, s in zip(training_state(tr, net), saved):
        t.copy_(s)
    net.prepare_filters()                          # (the data-gradient filter copies follow the bf16 filters)
    tr.global_step = step0
    skipped = int(tr.skipped_steps)
    tr.step()
    # the verdict over ALL ranks (every rank raises or none: a rank left behind would wait in the next collective)
    bad = torch.tensor([int(tr.skipped_steps) - skipped, int(tr.match_status().max() != 0)], dtype=torch.int32, device=net.W.device)
    if pg is not None:
        torch.distributed.all_reduce(bad, group=pg)
    if int(bad.sum()) != 0:
        raise RuntimeError("--dump-outputs: the step from the seeded state was not applied on every rank "
                           "(skipped on %d, matching failed on %d)" % tuple(bad.tolist()))
    if rank != 0:
        return
    os.makedirs(path, exist_ok=True)
    hw, hb = net.head_w_start, net.head_bt_start
    arrays = {"locs": net.locs, "logits": net.logits, "loc_gradients": net.d_locs, "logit_gradients": net.d_logits,
              "moving_mean": net.MM, "moving_variance": net.MV,
              "head_weight_gradients": net.Wg[hw:], "head_weights": net.W[hw:], "head_weights_ema": tr.Wema[hw:],
              "head_beta_gradients": net.Btg[hb:net.nBt], "head_beta": net.Bt[hb:]}
    for name, t in arrays.items():
        t = t.detach()
        idx = dump_indices(t.numel())
        if idx is not None:
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())
    np.save(os.path.join(path, "losses.npy"), np.array(tr.losses(), np.float64))


def launch_plan(gpus, env, argv, visible_devices, script=None, port=None):
    """What `--gpus N` means for THIS process (no GPU is touched here; decided before torch is imported):
      ("run", None)        -- this process is a rank (or the single-GPU run): go on
      ("spawn", [cmd...])  -- --gpus N > 1 and no rendezvous in the environment: start N ranks as a CHILD
                              `python -m torch.distributed.run` (never exec: a process that may have initialised the GPU
                              must not replace itself) and hand its exit code back
      ("refuse", message)  -- the request cannot be honoured: WORLD_SIZE disagrees with --gpus, or fewer than N devices are
                              visible.  A line labelled n_gpus: 1 under `--gpus 8` would be a void measurement."""
    world_env = env.get("WORLD_SIZE")
    if gpus < 1:
        return "refuse", "--gpus must be >= 1 (got %d)" % gpus
    if world_env is not None:
        if int(world_env) != gpus:
            return "refuse", ("WORLD_SIZE=%s (the launcher started that many ranks) but --gpus %d: refusing to print a line "
                              "whose n_gpus does not match the request" % (world_env, gpus))
        return "run", None
    if gpus == 1:
        return "run", None
    if visible_devices < gpus:
        return "refuse", "--gpus %d but only %d GPU(s) visible on this node: not starting ranks that would share a device" % (gpus, visible_devices)
    if port is None:
        import socket
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), script or os.path.abspath(__file__)] + list(argv)
    return "spawn", cmd


def spawn_ranks(cmd):
    """Run the N-rank job as a child process; its stdout (rank 0's ONE JSON line) and stderr pass straight through."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL over xGMI needs it on this host driver
    return subprocess.call(cmd, env=env)


def visible_gpu_count():
    """Devices visible to this process WITHOUT initialising the GPU (torch.cuda.device_count() does not, on this image)."""
    try:
        import torch
        return int(torch.cuda.device_count())
    except Exception:
        return 0


def usable_cores():
    """Host cores this process may actually use (affinity mask and cgroup CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(p))))
    except Exception:
        pass
    return n


def cpu_baseline(net, priors, seconds):
    """Restated CPU reference, config (i): --fine_tune, B=2, 299x299, k=5, G=13, all host cores."""
    import torch
    from oracle.cpu_train import CpuTrainer
    from multibox_amd.synth import synthetic_batch
    cores = usable_cores()
    torch.set_num_threads(cores)
    params = {n: net.get_param(n).detach().float().cpu().clone() for n in net.param_index}
    tr = CpuTrainer(params, priors, k=net.k, fine_tune=True)
    images, gt, n = synthetic_batch(2, net.S, 13, seed=0)
    images = torch.from_numpy(images)
    tr.step(images, gt, n)                      # warm-up
    t0, steps = time.time(), 0
    while steps < 2 or (time.time() - t0 < seconds and steps < 50):
        tr.step(images, gt, n)
        steps += 1
    dt = time.time() - t0
    return {"value": round(2 * steps / dt, 3), "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": "%d steps of train.py --fine_tune semantics, BATCH_SIZE=2, 299x299, k=5, torch-CPU fp32 restatement "
                      "(oracle/cpu_train.py; TF 0.11 cannot run here)" % steps}


def _conv_flops(d):
    if d.transposed:
        return 2.0 * d.N * d.H_in * d.W_in * d.C_in * d.R * d.S * d.C_out
    return 2.0 * d.N * d.H_out * d.W_out * d.C_out * d.R * d.S * d.C_in


# entry point -> (kernel class, algorithmic work of one call).  MFMA classes count FLOPs, HBM classes bytes
# (SURVEY 8d / DESIGN 4: bn apply reads y and writes a = 4 B per element; the one-launch bn backward reads da, y and
# writes dy = 6 B; the three-launch form reads da, y twice = 10 B).
def _work_table():
    W = {}
    W["mbx_conv"] = ("igemm", "mfma", lambda a: _conv_flops(a[0]._obj))
    W["mbx_conv_pair"] = ("igemm", "mfma", lambda a: _conv_flops(a[0]._obj) + _conv_flops(a[1]._obj))      # two sibling convs, one launch
    W["mbx_conv_wgrad_scaled"] = ("wgrad", "mfma", lambda a: _conv_flops(a[0]._obj))
    W["mbx_conv_wgrad_grouped"] = ("wgrad", "mfma", lambda a: float(a[1]._obj.flops))  # mbx_wgrad_plan_info.flops
    W["mbx_conv_wgrad_grouped_capped"] = W["mbx_conv_wgrad_grouped"]                    # (the entry point the engine calls)
    W["mbx_bn_apply_fused"] = ("bn_fwd", "hbm", lambda a: 4.0 * a[6] * a[7])
    # finalize + apply in one launch from the few statistics rows the convolution ADDED (a[6], a[7] = M, C)
    W["mbx_bn_apply_fused_mapped"] = ("bn_fwd", "hbm", lambda a: 4.0 * a[6] * a[7])
    W["mbx_bn_finalize"] = ("bn_fwd", "hbm", lambda a: 0.0)
    W["mbx_bn_finalize_parts"] = ("bn_fwd", "hbm", lambda a: 0.0)
    W["mbx_bn_apply_mapped"] = ("bn_fwd", "hbm", lambda a: 4.0 * a[1] * a[2])                  # a batch-norm group: [M, sum K]
    # normalise + 3x3/2 max-pool in one pass: y read once, pooled tensor + argmax bytes written (a[1..4] = N,H,W,C; a[12], a[13] = Ho, Wo)
    W["mbx_bn_apply_maxpool"] = ("bn_fwd", "hbm", lambda a: (2.0 * a[1] * a[2] * a[3] + 3.0 * a[1] * a[12] * a[13]) * a[4])
    W["mbx_bn_bwd_onepass"] = ("bn_bwd", "hbm", lambda a: 6.0 * a[4] * a[5])
    W["mbx_bn_bwd_onepass_mapped"] = ("bn_bwd", "hbm", lambda a: 6.0 * a[4] * a[5])
    W["mbx_bn_bwd_reduce"] = ("bn_bwd", "hbm", lambda a: 4.0 * a[6] * a[7])
    W["mbx_bn_bwd_apply"] = ("bn_bwd", "hbm", lambda a: 6.0 * a[6] * a[7])
    W["mbx_bn_bwd_reduce_mapped"] = ("bn_bwd", "hbm", lambda a: 4.0 * a[6] * a[7])
    W["mbx_bn_bwd_apply_mapped"] = ("bn_bwd", "hbm", lambda a: 6.0 * a[6] * a[7])
    # pooled forms (a[4..8] = N,H,W,Ho,Wo; a[11] = C): y (+ dy) per element, pool gradient + argmax per pooled element
    W["mbx_bn_bwd_reduce_pooled"] = ("bn_bwd", "hbm", lambda a: (2.0 * a[4] * a[5] * a[6] + 3.0 * a[4] * a[7] * a[8]) * a[11])
    W["mbx_bn_bwd_apply_pooled"] = ("bn_bwd", "hbm", lambda a: (4.0 * a[4] * a[5] * a[6] + 3.0 * a[4] * a[7] * a[8]) * a[11])
    W["mbx_bn_bwd_finalize"] = ("bn_bwd", "hbm", lambda a: 0.0)
    return W


def timed_eager_pass(run, entry_points=None):
    """HIP events around every call of the listed libmbx entry points during run() (an eager pass on the current
    stream), the GPU parked behind a spin kernel while the host queues ahead.  What the event markers themselves add is
    MEASURED, not assumed: the same pass is timed once more WITHOUT the per-launch events (one event pair around the whole
    pass, GPU parked the same way).  (instrumented - plain) / (2 x pairs) is the cost of ONE marker packet; the interval
    between a launch's two timestamps holds the kernel (dispatch to completion: what a rocprofv3 kernel trace reports)
    plus exactly one marker's processing, so one marker cost is subtracted from every interval.  Checked against the
    rocprofv3 kernel trace of the same build (profiles/README.md, round 3).  Round 2 subtracted the 5 us an EMPTY event
    pair reads, which over-corrected by ~1.3 us per launch: 0.163 printed against 0.145 from the trace.
    Returns ({class: dict(ms, raw_ms, work, calls, bound)}, cost of one marker in ms, plain pass in ms)."""
    import torch
    from multibox_amd import _lib
    l = _lib.lib()
    table = _work_table()
    names = [n for n in (entry_points or table) if hasattr(l, n)]
    recs = []
    orig = {n: getattr(l, n) for n in names}

    def wrap(name):
        cls, bound, work = table[name]
        fn = orig[name]

        def wrapped(*a):
            a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            r = fn(*a)
            b0.record()
            recs.append((cls, bound, float(work(a)), a0, b0))
            return r
        return wrapped

    def parked(fn):
        # Park the GPU behind a ~40 ms spin kernel while the host enqueues the pass: otherwise the GPU idles inside every
        # event pair waiting for the next eager launch (host launch latency ~5 us per kernel)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda._sleep(int(40e-3 * 2.0e9))
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)
    plain_ms = min(parked(run) for _ in range(2))
    for n in names:
        setattr(l, n, wrap(n))
    try:
        inst_ms = parked(run)
    finally:
        for n in names:
            setattr(l, n, orig[n])
    pair_ms = max(inst_ms - plain_ms, 0.0) / max(2 * len(recs), 1)       # one marker
    out = {}
    for cls, bound, work, a, b in recs:
        o = out.setdefault(cls, dict(ms=0.0, raw_ms=0.0, work=0.0, calls=0, bound=bound))
        dt = a.elapsed_time(b)
        o["raw_ms"] += dt
        o["ms"] += max(dt - pair_ms, 0.0)
        o["work"] += work
        o["calls"] += 1
    return out, pair_ms, plain_ms


# (the pair launch runs two igemm3 problems in one grid; the split-K reduce launch is the epilogue of its igemm3 slices)
# (... and conv_direct3_kernel is the same convolution -- forward + data gradient of the stem's 3x3 layers -- as a direct launch)
KERNEL_CLASSES = (("igemm", ("conv_igemm3_kernel", "conv_igemm3_pair_kernel", "conv_igemm5_kernel", "conv_igemm7_kernel",
                             "conv_direct3_kernel", "conv_directw_kernel", "conv_resident_kernel", "conv_pwres_kernel", "conv_stem_kernel", "splitk_reduce_kernel")), ("wgrad", ("conv_wgrad",)),
                  ("bn_fwd", ("bn_finalize_kernel", "bn_finalize_parts_kernel", "bn_apply_kernel", "bn_apply_fused_kernel",
                              "bn_apply_rows_kernel", "bn_apply_maxpool3s2_kernel")), ("bn_bwd", ("bn_bwd_",)))


EXPECT_IGEMM_LAUNCHES = [0]      # convolution-class launches of one step (set from the eager pass before the trace is taken)


def traced_kernel_times(step_fn, steps=3):
    """Per-kernel-class GPU time of `steps` REAL steps (hipGraph replays included) from the kernels' own begin / end
    timestamps, recorded live by the ROCm tracer through torch.profiler -- the same timestamps a `rocprofv3
    --kernel-trace` run of this command reports, so `roofline.frac` can be recomputed from the committed
    profiles/r03_*_kernel_stats.csv.  (HIP-event intervals around eager launches, round 1-2's method, carry a marker
    packet each whose cost depends on the kernel's length: they read 3 % low on the 23 us convolution launches and
    20 % low on the 5 us batch-norm launches after any constant correction; kept as a cross-check field.)
    Returns {class: (ms per step, launches per step)} or None if the tracer is unavailable."""
    import torch
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                step_fn()
            torch.cuda.synchronize()
        out = {}
        seen = 0
        allk = [0.0, 0]
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        evs.sort(key=lambda e: e.time_range.start)
        # The tracer can lose the first kernels after it starts: cut the trace into steps at pack_input_kernel (the first kernel of
        # a step) and keep the steps that have every kernel (the longest ones); what precedes the first marker is a torn step.
        marks = [i for i, e in enumerate(evs) if "pack_input" in e.name]
        if marks:
            segs = [evs[a:b] for a, b in zip(marks, marks[1:] + [len(evs)])]
            full = max(len(sg) for sg in segs)
            segs = [sg for sg in segs if len(sg) == full]
            evs, steps = [e for sg in segs for e in sg], len(segs)
        for e in evs:
            seen += 1
            us = float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))
            if "Memcpy" not in e.name and "Memset" not in e.name:
                allk[0] += us
                allk[1] += 1
            for cls, keys in KERNEL_CLASSES:
                if any(k in e.name for k in keys):
                    o = out.setdefault(cls, [0.0, 0])
                    o[0] += us
                    o[1] += 1
                    break
        if not seen or "igemm" not in out:
            return None
        out["_all_kernels"] = allk                       # every kernel of the traced steps (optimiser launches included)
        out = {c: (v[0] / steps * 1e-3, v[1] / float(steps)) for c, v in out.items()}
        out["_steps"] = (float(steps), float(steps))      # complete steps the figures are averaged over
        return out
    except Exception:
        return None


def _file_sha(path):
    import hashlib
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def committed_traffic(pattern="r*_hbm_traffic_pmc.json"):
    """HBM bytes per launch of the dominant kernel class (conv_igemm3_kernel + conv_igemm5_kernel + conv_igemm7_kernel launches,
    weighted by their launch counts) from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes -- only if that profile was
    taken on THESE kernel sources (the file stamps the sha256 of csrc/conv.hip, conv5.hip and conv7.hip); a stale profile prints null."""
    import glob
    shas = {k: _file_sha(os.path.join(ROOT, "multibox_amd", "csrc", f)) for k, f in (("conv_hip_sha", "conv.hip"), ("conv5_hip_sha", "conv5.hip"), ("conv7_hip_sha", "conv7.hip"),
                                                                                  ("convd_hip_sha", "convd.hip"), ("convr_hip_sha", "convr.hip"), ("conv_common_h_sha", "conv_common.h"))}
    for pj in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
        try:
            j = json.load(open(pj))
            if any(j.get(k) != v for k, v in shas.items()):
                continue
            n = mb = 0.0
            for kern in ("conv_igemm3_kernel", "conv_igemm3_pair_kernel", "conv_igemm5_kernel", "conv_igemm7_kernel", "conv_direct3_kernel", "conv_directw_kernel", "conv_resident_kernel", "conv_pwres_kernel", "conv_stem_kernel"):
                if kern in j:
                    n += j[kern]["calls"]
                    mb += j[kern]["calls"] * j[kern]["MB_per_launch"]
            if n <= 0:
                continue
            return mb / n * 1e6, os.path.relpath(pj, ROOT) + \
                " (launch-weighted mean over conv_igemm3 / pair / igemm5 / igemm7 / direct3 launches; FETCH_SIZE x2 gfx950 correction + " \
                "WRITE_SIZE, separate --pmc passes; source shas match)"
        except Exception:
            continue
    return None, "no committed PMC profile matches the current csrc/conv*.hip + conv_common.h (%s)" % shas


def committed_kernel_traffic(kernel, ms_per_launch, pattern="r*_hbm_traffic_pmc.json"):
    """HBM bytes per launch of one kernel from the newest committed PMC profile that has it, and the rate at the given duration."""
    import glob
    for pj in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
        try:
            j = json.load(open(pj))
            if kernel in j and ms_per_launch > 0:
                mb = float(j[kernel]["MB_per_launch"])
                gbs = mb * 1e6 / (ms_per_launch * 1e-3) / 1e9
                return {"traffic_MB_per_launch": round(mb, 1), "GB/s": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                        "source": os.path.relpath(pj, ROOT)}
        except Exception:
            continue
    return None


def roofline_objects(classes, pair_ms, plain_ms, whole_step_tflops=None, dominant="igemm", traced=None):
    """(roofline of the dominant kernel, list of per-class rooflines).  Work (FLOPs / bytes) and launch counts come
    from timed_eager_pass(); times from traced_kernel_times() when the tracer is available (then `ms` is the tracer's and
    `event_ms` the HIP-event figure), else from the HIP events."""
    classes = {c: o for c, o in classes.items() if not c.startswith("_")}
    for cls, o in classes.items():
        o["event_ms"] = o["ms"]
        o["traced_launches"] = None
        if traced is not None and cls in traced:
            o["ms"] = traced[cls][0]
            o["traced_launches"] = traced[cls][1]
    # The tracer can LOSE events (round 4's step trace had a 3 ms hole; torch.profiler over graph replays has been seen to report 391
    # of 399 convolution kernels, every step alike): time summed over fewer launches than the step makes would print an inflated
    # fraction.  A complete trace shows at least as many kernels of the dominant class as the eager pass counted calls (pair
    # launches are one call and one kernel; split-K is one call and two kernels).  An incomplete one (after the retries of
    # main()) is NOT used: `frac` / `achieved` are then null (the tracer's figure is kept under `incomplete_trace`, the HIP-event
    # figure under `frac_hip_events`).
    d = classes[dominant]
    tl = d.get("traced_launches")
    traced_ok = traced is None or tl is None or tl >= d["calls"] - 0.5
    incomplete = None
    if not traced_ok:
        incomplete = {"ms_per_step": round(d["ms"], 3), "frac": round(d["work"] / (d["ms"] * 1e-3) / 1e12 / MFMA_BF16_DENSE_PEAK_TFLOPS, 4),
                      "traced_launches_per_step": round(tl, 2)}
    kernels = []
    for cls, o in sorted(classes.items()):
        if o["ms"] <= 0 or o["work"] <= 0:
            continue
        if o["bound"] == "mfma":
            ach, peak, unit = o["work"] / (o["ms"] * 1e-3) / 1e12, MFMA_BF16_DENSE_PEAK_TFLOPS, "TFLOP/s"
        else:
            ach, peak, unit = o["work"] / (o["ms"] * 1e-3) / 1e9, HBM_PEAK_GBS, "GB/s"
        kernels.append({"kernel": cls, "bound": o["bound"], "achieved": round(ach, 2), "peak": peak, "unit": unit,
                        "frac": round(ach / peak, 4), "launches": o["calls"], "ms_per_step": round(o["ms"], 3),
                        "avg_launch_us": round(1e3 * o["ms"] / o["calls"], 2), "ms_per_step_hip_events": round(o["event_ms"], 3)})
        if cls == "wgrad":
            # the grouped weight gradient reads every convolution input and every output gradient of the step once: beside its
            # MFMA fraction, the HBM rate of the launch from the committed PMC passes (FETCH_SIZE x2 + WRITE_SIZE per launch)
            kernels[-1]["hbm"] = committed_kernel_traffic("conv_wgrad_grouped_kernel", o["ms"] / o["calls"])
    d = classes[dominant]
    ach = d["work"] / (d["ms"] * 1e-3) / 1e12
    traffic, src = committed_traffic()
    main = {"bound": "mfma", "kernel": "conv_igemm3_kernel (+ pair, split-K slices and their reduce) + conv_igemm5_kernel + conv_igemm7_kernel + conv_direct3_kernel + conv_directw_kernel + conv_resident_kernel + conv_pwres_kernel + conv_stem_kernel (convolution on MFMA: forward + data-gradient launches)",
            "achieved": round(ach, 2) if traced_ok else None, "peak": MFMA_BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / MFMA_BF16_DENSE_PEAK_TFLOPS, 4) if traced_ok else None, "traffic": traffic, "traffic_source": src,
            "launches_per_step": d["calls"], "traced_launches_per_step": (round(tl, 2) if tl is not None else None),
            "traced_complete": bool(traced_ok), "incomplete_trace": (None if traced_ok else incomplete), "avg_launch_us": round(1e3 * d["ms"] / d["calls"], 2),
            "ms_per_step": round(d["ms"], 3),
            "timing": ("kernel begin/end timestamps of 3 real (graph-replayed) steps, recorded live by the ROCm tracer via "
                       "torch.profiler: the timestamps of a rocprofv3 kernel trace (profiles/r06_bench_b64_kernel_stats.csv)"
                       if traced is not None else
                       "HIP events around every launch of one eager pass minus one measured marker cost per interval "
                       "(tracer unavailable or its trace incomplete: traced_complete)"),
            "frac_hip_events": round(d["work"] / (d["event_ms"] * 1e-3) / 1e12 / MFMA_BF16_DENSE_PEAK_TFLOPS, 4),
            "event_marker_us": round(1e3 * pair_ms, 2), "eager_pass_ms": round(plain_ms, 3),
            "frac_raw_event_intervals": round(d["work"] / (d["raw_ms"] * 1e-3) / 1e12 / MFMA_BF16_DENSE_PEAK_TFLOPS, 4),
            "algorithmic_gflop_per_launch": round(d["work"] / d["calls"] / 1e9, 3)}
    if whole_step_tflops is not None:
        main["whole_step_frac"] = round(whole_step_tflops / MFMA_BF16_DENSE_PEAK_TFLOPS, 4)   # all 5.1 TFLOP of the step / its wall time
    return main, kernels


def detect_leg(args, world, rank, pg):
    """BASELINE config 4: the detect.py path -- inference-mode forward (frozen BN, bf16) + sigmoid + decode / clip /
    filter / top-K / convert at BATCH_SIZE=256 patches per GPU, k=7 (P=904), whole-image restrictions, max_to_keep
    200.  Patches shard over ranks with no collective; value = all ranks' patches / max-over-ranks time."""
    import numpy as np
    import torch
    from multibox_amd.engine import Net
    from multibox_amd import priors as PR, detect as D, _lib
    from multibox_amd.synth import DEFAULT_ASPECT_RATIOS
    B, k, S = args.detect_batch, 7, 299
    priors = np.array(PR.generate_priors(DEFAULT_ASPECT_RATIOS[k]), np.float32)
    net = Net(batch=B, input_size=S, k=k, mode="infer", seed=2)
    net.fold_bn()
    gen = torch.Generator().manual_seed(1000 + rank)
    images = (torch.rand(B, S, S, 3, generator=gen) * 2 - 1).cuda()
    meta = D.make_patch_meta(np.zeros((B, 2), np.int32), np.tile([[S, S]], (B, 1)), np.zeros((B, 1), np.int32),
                             np.tile([[0., 0., 1., 1.]], (B, 1)), np.full((B, 1), 200), np.tile([[S, S]], (B, 1)))
    pp = D.DetectPostprocess(priors, B, k_max=200)
    conf = torch.empty((B, net.P), device="cuda")
    l = _lib.lib()

    def one():
        net.set_input(images)
        net.forward()
        _lib.check(l.mbx_decode_conf(None, net.logits.data_ptr(), None, B, net.P, 0.0, None, conf.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "sigmoid")
        pp(net.locs, conf, meta)
    for _ in range(2):
        one()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        one()
    for _ in range(3):
        gr.replay()

    def sync():
        if pg is not None:
            torch.distributed.barrier()
        torch.cuda.synchronize()
    n = args.detect_steps
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        gr.replay()
    sync()
    dt = time.perf_counter() - t0
    if pg is not None:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)
    count_ok = bool((pp.count == 200).all())
    out = {"metric": "images/sec detect (299x299 patches, 7-AR priors, P=%d): forward + decode/clip/filter/top-K/convert" % net.P,
           "value": round(B * world * n / dt, 1), "unit": "images/sec", "ms_per_batch": round(1e3 * dt / n, 3), "steps": n,
           "config": {"workload": "detect.py path, BASELINE config 4: BATCH_SIZE=%d patches/GPU, k=7 (P=%d), restrictions "
                                  "[0,0,1,1], max_to_keep 200, inference BN, bf16 storage" % (B, net.P),
                      "global_batch": B * world, "parallelism": "dp%d (patches sharded, no collective)" % world},
           "all_patches_kept_200": count_ok}
    if rank == 0 and not args.no_roofline:
        try:
            classes, pair_ms, _ = timed_eager_pass(one, ["mbx_conv"])
            d = classes["igemm"]
            ach = d["work"] / (d["ms"] * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": "conv_igemm3_kernel + conv_igemm5_kernel + conv_igemm7_kernel + conv_direct3_kernel + conv_directw_kernel + conv_resident_kernel + conv_pwres_kernel + conv_stem_kernel (forward, folded-BN epilogue)", "achieved": round(ach, 2),
                               "peak": MFMA_BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / MFMA_BF16_DENSE_PEAK_TFLOPS, 4),
                               "traffic": None, "launches_per_batch": d["calls"], "avg_launch_us": round(1e3 * d["ms"] / d["calls"], 2)}
            # HBM bytes per launch from the committed PMC passes of the detect forward (tools/collect_profiles.sh part d), if taken on these sources
            out["roofline"]["traffic"], out["roofline"]["traffic_source"] = committed_traffic("r*_detect_traffic_pmc.json")
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                pp(net.locs, conf, meta)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) / 20 * 1e3
            alg = B * (20.0 * net.P + 24.0 * 200)                       # 20 B x P read + 24 B x K written per patch
            out["postprocess"] = {"kernel": "decode_filter_topk_kernel", "bound": "hbm (launch-latency in practice)",
                                  "us_per_batch": round(us, 1), "achieved": round(alg / us / 1e3, 2), "peak": HBM_PEAK_GBS,
                                  "unit": "GB/s", "frac": round(alg / us / 1e3 / HBM_PEAK_GBS, 5)}
            # BASELINE config 4 names a per-image NMS; the reference has none, so it is an OPTIONAL stage that
            # is NOT part of `value` above: timed here on the same batch for the record (mbx_nms, IoU 0.5)
            ppn = D.DetectPostprocess(priors, B, k_max=200, nms_iou=0.5)
            ppn(net.locs, conf, meta)
            a.record()
            for _ in range(20):
                ppn(net.locs, conf, meta)
            b.record()
            torch.cuda.synchronize()
            out["optional_nms"] = {"kernel": "decode_filter_topk_kernel + nms_kernel", "iou_threshold": 0.5,
                                   "us_per_batch": round(a.elapsed_time(b) / 20 * 1e3, 1),
                                   "mean_kept_of_200": round(float(ppn.count.float().mean()), 1),
                                   "note": "not in the reference (detect.py:408-443 has no NMS); not included in value"}
        except Exception as e:
            out["roofline"] = {"error": repr(e)}
    del gr
    return out


def config_leg(args, fine_tune, input_size, k, max_num_bboxes, label, env=None):
    """One more single-GPU BASELINE configuration beside the headline, same build, same timing rules (inputs resident,
    barrier-free single rank, --config-steps timed steps after 3 warm-up steps): `--fine_tune` at BATCH_SIZE 64 (BASELINE
    config 1's semantics at the headline's batch: the like-for-like partner of cpu_baseline) or the 512x512 / k=7 /
    MAX_NUM_BBOXES=100 geometry of config 5.  roofline = the implicit-GEMM launches of three traced replayed steps."""
    import numpy as np
    import torch
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer, decay_steps
    from multibox_amd import priors as PR
    from multibox_amd.synth import synthetic_batch, DEFAULT_ASPECT_RATIOS
    B = args.batch
    priors = PR.priors_for_input_size(DEFAULT_ASPECT_RATIOS[k], input_size).astype(np.float32)
    old_env = {k_: os.environ.get(k_) for k_ in (env or {})}
    os.environ.update(env or {})                   # (engine switches are read when the network is built)
    try:
        net = Net(batch=B, input_size=input_size, k=k, mode="train", fine_tune=fine_tune, seed=2)
    finally:
        for k_, v_ in old_env.items():
            if v_ is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v_
    tr = Trainer(net, priors, max_num_bboxes=max_num_bboxes, location_loss_alpha=1000.0, decay_steps_=decay_steps(56945, B, 4),
                 use_graph=not args.no_graph)
    images, gt, n = synthetic_batch(B, input_size, max_num_bboxes, seed=0)
    tr.set_batch(torch.from_numpy(images).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n).cuda())
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.config_steps):
        tr.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.config_steps
    losses = tr.losses()
    gflop = net.flops_per_image(train=True) * 1e-9
    out = {"workload": label, "value": round(B / dt, 1), "unit": "images/sec", "ms_per_step": round(1e3 * dt, 3), "steps": args.config_steps,
           "batch": B, "predictions": net.P, "algorithmic_tflop_per_step": round(gflop * B * 1e-3, 3),
           "model_tflops": round(gflop * B * 1e-3 / dt, 1), "matching_ok": int(tr.match_status().max()) == 0,
           "grid_barrier_timeouts": net.barrier_timeouts(), "total_loss_finite": bool(np.isfinite(losses[3])),
           "fused_conv_bn_apply_launches": net.fused_apply_launches, "fused_dgrad_bn_backward_launches": net.fused_bwd_launches,
           "bn_layers_without_a_backward_launch": net.fused_bwd_layers}
    if not args.no_roofline:
        try:
            traced = traced_kernel_times(tr.step)
            if traced is not None and "_all_kernels" in traced:
                out["kernels_per_step"] = round(traced["_all_kernels"][1], 1)
            classes, pair_ms, plain_ms = timed_eager_pass(tr.run_eager_once, ["mbx_conv"])
            d = classes["igemm"]
            ms = traced["igemm"][0] if traced else d["ms"]
            ach = d["work"] / (ms * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": "implicit-GEMM convolution launches (forward + data gradient)",
                               "achieved": round(ach, 2), "peak": MFMA_BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(ach / MFMA_BF16_DENSE_PEAK_TFLOPS, 4), "launches_per_step": d["calls"],
                               "ms_per_step": round(ms, 3), "timing": "tracer" if traced else "hip events",
                               "whole_step_frac": round(out["model_tflops"] / MFMA_BF16_DENSE_PEAK_TFLOPS, 4), "traffic": None}
        except Exception as e:
            out["roofline"] = {"error": repr(e)}
    del tr, net
    torch.cuda.empty_cache()
    return out


def input_leg():
    """Row F1/F3 beside the headline: the GPU half of the training input (mbx_augment_batch: resize by the drawn method,
    colour ops, flip, scaling) on one batch of 64 synthetic 480x640 uint8 pictures ALREADY in HBM, every method and
    colour ordering present -- images/s and algorithmic bytes (3 B per source pixel read + 12 B per output pixel
    written) against the HBM peak.  Not part of `value`."""
    import numpy as np
    import torch
    from multibox_amd import _lib, inputs as I
    from multibox_amd.augment import BatchAugmenter
    B, S, H, W = 64, 299, 480, 640
    rng = np.random.RandomState(0)
    aug = BatchAugmenter(B, S, slot_bytes=H * W * 3)
    aug.begin()
    u8 = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    for i in range(B):
        aug.add(u8, i % 4, i % 2, I.color_ops(i % 4, False, rng) if i % 3 else [])
    aug.run()                                                     # uploads the sources once; the timed part is launches only
    torch.cuda.synchronize()
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        _lib.check(L.mbx_augment_batch(aug.d_pix.data_ptr(), aug.d_items.data_ptr(), B, S, int(aug.any_contrast),
                                       aug.out.data_ptr(), aug.workspace.data_ptr(), st), "mbx_augment_batch")
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / 20 * 1e3
    alg = B * (3.0 * H * W + 12.0 * S * S)
    return {"kernel": "augment_resize_kernel + augment_sums_kernel + augment_color_kernel", "bound": "hbm",
            "workload": "64 x (480x640 uint8 -> 299x299x3 f32), methods 0..3, four colour orderings, flips",
            "us_per_batch": round(us, 1), "images_per_s": round(B / us * 1e6, 0), "achieved": round(alg / us / 1e3, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / us / 1e3 / HBM_PEAK_GBS, 4),
            "note": "inputs resident in HBM; with the upload (59 MB over PCIe) 1.4 ms per batch, see DESIGN.md"}


def main():
    args = parse()
    # --gpus N: start N ranks (one per GPU, RCCL) unless a launcher already did -- decided before anything touches the GPU
    need_count = args.gpus > 1 and "WORLD_SIZE" not in os.environ
    action, what = launch_plan(args.gpus, os.environ, sys.argv[1:], visible_gpu_count() if need_count else 0)
    if action == "refuse":
        print("bench.py: " + what, file=sys.stderr)
        raise SystemExit(2)
    if action == "spawn":
        raise SystemExit(spawn_ranks(what))
    import numpy as np
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    torch.cuda.set_device(local_rank)
    pg = None
    if world > 1 or os.environ.get("MBX_FORCE_DIST"):       # MBX_FORCE_DIST: exercise the RCCL path on one GPU
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        pg = dist.group.WORLD
    import __graft_entry__ as g
    if local_rank == 0:
        g.build()
    if pg is not None:
        torch.distributed.barrier()
    # evidence that the process group is RCCL and really spans `world` ranks: an all-reduce of ones
    rccl = {"backend": None, "ranks": 1, "allreduce_of_ones": 1}
    if pg is not None:
        ones = torch.ones(1, device="cuda")
        torch.distributed.all_reduce(ones)
        rccl = {"backend": torch.distributed.get_backend(pg), "ranks": torch.distributed.get_world_size(pg),
                "allreduce_of_ones": int(ones)}
    # the line's n_gpus is what --gpus asked for, and the process group really spans that many ranks
    assert world == args.gpus and rccl["ranks"] == args.gpus and rccl["allreduce_of_ones"] == args.gpus, (world, args.gpus, rccl)
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer, decay_steps
    from multibox_amd import priors as PR
    from multibox_amd.synth import synthetic_batch, DEFAULT_ASPECT_RATIOS

    B = args.batch
    ars = DEFAULT_ASPECT_RATIOS[args.k]
    priors = PR.priors_for_input_size(ars, args.input_size).astype(np.float32)
    from multibox_amd.dist import bn_max_workgroups_for
    # N>1: leave the CUs RCCL's channels can hold to the collectives of the bucket in flight (derived, not a constant)
    bn_cap, bn_cap_why = bn_max_workgroups_for(world, torch.cuda.get_device_properties(local_rank).multi_processor_count)
    net = Net(batch=B, input_size=args.input_size, k=args.k, mode="train", fine_tune=args.fine_tune, seed=2,
              bn_max_workgroups=bn_cap)
    tr = Trainer(net, priors, max_num_bboxes=args.max_num_bboxes, location_loss_alpha=1000.0,
                 decay_steps_=decay_steps(56945, B * world, 4), use_graph=not args.no_graph, process_group=pg)
    images, gt, n = synthetic_batch(B, args.input_size, args.max_num_bboxes, seed=100 * rank)    # each rank its own shard
    tr.set_batch(torch.from_numpy(images).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n).cuda())
    seeded_state = (tr.global_step, [t.clone() for t in training_state(tr, net)]) if args.dump_outputs else None

    def sync():
        if pg is not None:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        tr.step()
        if args.log_losses and rank == 0:
            print("warmup step %d losses (loc, conf, reg, total) %s" % (tr.global_step, tr.losses()), file=sys.stderr)
    sync()
    if pg is not None:
        tr.exposed_events = []                 # step() brackets reducer.wait() with an event pair: the all-reduce time nothing hides
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.step()
        if args.log_losses and rank == 0:
            print("step %d losses (loc, conf, reg, total) %s" % (tr.global_step, tr.losses()), file=sys.stderr)
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0          # this rank alone (before the closing barrier)
    sync()
    dt = time.perf_counter() - t0
    roofline = args.full and not args.no_roofline
    dp_diag = None
    if pg is not None:
        exposed = [a.elapsed_time(b) for a, b in tr.exposed_events]
        tr.exposed_events = None
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)
        # per-rank figures -> max / min over ranks (two small collectives, outside the timed region)
        mine = torch.tensor([dt_own / args.steps * 1e3, sum(exposed) / max(len(exposed), 1), max(exposed or [0.0])],
                            dtype=torch.float64, device="cuda")
        hi, lo = mine.clone(), mine.clone()
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        dp_diag = {"rank_step_ms_max": round(float(hi[0]), 3), "rank_step_ms_min": round(float(lo[0]), 3),
                   "allreduce_exposed_ms": round(float(hi[1]), 3), "allreduce_exposed_ms_min_rank": round(float(lo[1]), 3),
                   "allreduce_exposed_ms_worst_step": round(float(hi[2]), 3),
                   "buckets_bytes": [4 * (h - l) for _, l, h in tr._segments],
                   "last_bucket_carries": "beta gradients + step control block (%d bytes)" % (4 * (net.nBt + 8)),
                   "weight_gradient_overlap_cus": tr.overlap_cus,
                   "grid_barrier_workgroup_cap": bn_cap, "cus_left_to_rccl": bn_cap_why}
    losses = tr.losses()
    # health over ALL ranks: matching status and grid-barrier timeouts of the last step (summed)
    health = torch.tensor([int(tr.match_status().max() != 0), net.barrier_timeouts()], dtype=torch.int32, device="cuda")
    if pg is not None:
        torch.distributed.all_reduce(health)
    status_ok, barrier_timeouts = int(health[0]) == 0, int(health[1])
    # the trainer's own verdict (a collective: every rank): skipped steps, fall-back of the BN backward taken or not
    try:
        verdict = tr.check_health()
        verdict["error"] = None
    except RuntimeError as e:
        verdict = {"stop": False, "fallback": False, "error": str(e)}
    out = None
    if rank == 0:
        ms = 1e3 * dt / args.steps
        # SURVEY 8(d) figures for the BASELINE geometry; other geometries are counted from the network's own layers
        per_image_gflop = ((27.3 if args.fine_tune else 79.9) if (args.input_size, args.k) == (299, 5)
                           else net.flops_per_image() * 1e-9)
        value = B * world * args.steps / dt
        out = {"metric": "images/sec (%dx%d, %d-AR priors) train" % (args.input_size, args.input_size, args.k), "value": round(value, 2), "unit": "images/sec",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
               "data": "synthetic",
               "config": {"workload": "full train step: Inception-ResNet-v2 + multibox heads fwd, on-device matching+loss, bwd, "
                                      "RMSProp+EMA; %dx%d, k=%d (P=%d), BATCH_SIZE=%d/GPU, MAX_NUM_BBOXES=%d%s"
                                      % (args.input_size, args.input_size, args.k, net.P, B, args.max_num_bboxes,
                                         ", --fine_tune" if args.fine_tune else ""),
                          "global_batch": B * world, "parallelism": "dp%d" % world, "hip_graph": not args.no_graph},
               "final_losses": {"location": round(losses[0], 3), "confidence": round(losses[1], 3), "regularization": round(losses[2], 4)},
               "matching_ok": status_ok, "grid_barrier_timeouts": barrier_timeouts, "rccl": rccl,
               "health": {"fallback_taken_at_end": bool(verdict["fallback"]) or bool(net.no_onepass and not net.deterministic),
                          "skipped_steps": int(tr.skipped_steps), "error": verdict["error"], "events": list(tr.events)},
               # the kernel mix of THIS run (data-parallel runs cap the BN-backward grid; both use the same conv kernels)
               "kernels": {"igemm5_launches": sum(1 for _, d_, _ in net.tune_registry if 32 < d_.tile_config < 64),
                           "igemm7_launches": sum(1 for _, d_, _ in net.tune_registry if d_.tile_config == 65),
                           "split_k_launches": sum(1 for _, d_, _ in net.tune_registry if d_.tile_config > 128),
                           "fused_conv_bn_apply_launches": net.fused_apply_launches,
                           "fused_dgrad_bn_backward_launches": net.fused_bwd_launches, "bn_layers_without_a_backward_launch": net.fused_bwd_layers,
                           "bn_groups": len(net.bn_groups), "pair_launches": sum(int(g_.pair_fwd) + int(g_.pair_bwd) for g_ in net.bn_groups),
                           "fused_stem_pools": sum(1 for c_ in net.convs if getattr(c_, "fused_pool", None) is not None),
                           "backward_segments": len(tr._segments), "graphs": len(tr.graphs or []),
                           "bn_backward": "three-launch" if net.no_onepass else "one-launch (grid barrier, max %s workgroups)" % (net.bn_max_wg or "all"),
                           "skipped_steps_events": tr.events},
               "algorithmic_tflop_per_step": round(per_image_gflop * 1e-3 * B * world, 3)}
        out["model_tflops"] = round(out["algorithmic_tflop_per_step"] / (dt / args.steps), 2)
        if dp_diag is not None:
            out["data_parallel"] = dp_diag
        from multibox_amd import ops as _ops
        out["tune_cache"] = dict(_ops.TUNE_STATS)      # table entries accepted as they are / shapes measured on THIS box / refused
    if args.dump_outputs:                      # (after the line's losses and health are read: it takes one more step)
        dump_outputs(args.dump_outputs, tr, net, seeded_state, rank, pg)
        del seeded_state
    traced = None
    eager = None
    if roofline and rank == 0:
        try:
            eager = timed_eager_pass(tr.run_eager_once)       # (work and launch counts per kernel class; also what a complete trace must show)
            EXPECT_IGEMM_LAUNCHES[0] = eager[0]["igemm"]["calls"]
        except Exception as e:
            eager = e
    if roofline:                            # three more real steps on EVERY rank (the all-reduce needs them all); rank 0 traces its kernels
        if rank == 0:
            done = [0]

            def counted_step():
                tr.step()
                done[0] += 1
            traced = traced_kernel_times(counted_step)
            while done[0] < 3:          # the tracer gave up part-way: the other ranks still wait in three rounds of all-reduces
                counted_step()
            torch.cuda.synchronize()
            # a trace that lost events (fewer convolution kernels per step than the step launches: roofline_objects checks it) is
            # taken again -- single GPU only: with a process group every rank would have to repeat the same number of steps
            for _ in range(2):
                if pg is not None or traced is None or traced.get("igemm", (0, 1e9))[1] >= EXPECT_IGEMM_LAUNCHES[0] - 0.5:
                    break
                traced = traced_kernel_times(tr.step)
                torch.cuda.synchronize()
        else:
            for _ in range(3):
                tr.step()
            torch.cuda.synchronize()
    if roofline and rank == 0:
        try:
            if isinstance(eager, Exception):
                raise eager
            classes, pair_ms, plain_ms = eager
            out["roofline"], out["roofline_kernels"] = roofline_objects(classes, pair_ms, plain_ms, out["model_tflops"], traced=traced)
            if traced is not None and "_all_kernels" in traced:
                # every kernel of a replayed step + its eager optimiser launches, from the same trace
                out["kernels_per_step"] = round(traced["_all_kernels"][1], 1)
                out["kernel_time_ms_per_step"] = round(traced["_all_kernels"][0], 3)
                out["roofline"]["traced_steps"] = int(traced.get("_steps", (3, 3))[0])    # complete steps of the live trace
        except Exception as e:      # evidence only; never fail the benchmark line on it
            out["roofline"] = {"error": repr(e)}
    if pg is not None:
        torch.distributed.barrier()
    cpu_base = None
    if rank == 0 and args.full and not args.no_cpu_baseline and world == 1:
        try:
            cpu_base = cpu_baseline(net, priors, args.cpu_seconds)
        except Exception as e:
            cpu_base = {"error": repr(e)}
    del tr, net                     # free the training buffers before the other networks are built
    torch.cuda.empty_cache()
    if args.full and not args.no_detect:
        try:
            dleg = detect_leg(args, world, rank, pg)
        except Exception as e:
            dleg = {"error": repr(e)}
        if rank == 0:
            out["detect"] = dleg
            try:
                out["input_augment"] = input_leg()
            except Exception as e:
                out["input_augment"] = {"error": repr(e)}
        if pg is not None:
            torch.distributed.barrier()
    if rank == 0 and world == 1 and args.full and not args.no_configs and not args.fine_tune and (args.input_size, args.k) == (299, 5):
        cfgs = {}
        for key, ft, S_, k_, G_, label in (
                ("fine_tune", True, 299, 5, 13, "train.py --fine_tune (frozen backbone, heads train: BASELINE config 1's semantics), "
                                                "299x299, k=5, BATCH_SIZE=%d" % args.batch),
                ("s512_k7_g100", False, 512, 7, 100, "full train step at BASELINE config 5's geometry on one GPU: 512x512, k=7, "
                                                     "MAX_NUM_BBOXES=100, BATCH_SIZE=%d" % args.batch),
                # the headline configuration once more with round 6's FUSED launches (convolution + BN apply, data gradient + BN
                # backward behind in-kernel grid barriers: MBX_FUSE_APPLY=1 MBX_FUSE_BWD=1) -- built, bit-identical / parity-tested,
                # measured level and therefore OFF in `value`: this leg is the A/B on the driver's own box
                ("fused_launches", False, 299, 5, 13, "the headline step with the fused conv + BN launches ON (MBX_FUSE_APPLY=1 "
                                                      "MBX_FUSE_BWD=1; off in `value`), BATCH_SIZE=%d" % args.batch)):
            try:
                cfgs[key] = config_leg(args, ft, S_, k_, G_, label,
                                       env={"MBX_FUSE_APPLY": "1", "MBX_FUSE_BWD": "1"} if key == "fused_launches" else None)
            except Exception as e:
                cfgs[key] = {"error": repr(e)}
        out["configs"] = cfgs
        from multibox_amd import ops as _ops
        out["tune_cache"] = dict(_ops.TUNE_STATS)
    if rank == 0:
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
            if isinstance(out.get("configs", {}).get("fine_tune"), dict) and "value" in out["configs"]["fine_tune"]:
                # the like-for-like GPU figure sits beside it; the ratio is not a quality measure (roofline.frac is)
                cpu_base["same_semantics_on_gpu"] = "configs.fine_tune: %s images/sec at BATCH_SIZE %d" % (
                    out["configs"]["fine_tune"]["value"], args.batch)
        print(json.dumps(out), flush=True)
    if pg is not None:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
