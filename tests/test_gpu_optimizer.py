"""GPU: the optimiser choice (mbx_sgd_ema_step, mbx_adam_ema_step, Trainer(optimizer=...), the checkpoint) against the oracles of
tests/test_optimizer_cpu.py.

Bars.  Updates: rtol 1e-5 / atol 1e-6 against the float64 oracle, the optimiser bar of tests/test_gpu_grad_clip.py; a float32
numpy restatement alone meets it on this very data (test_optimizer_cpu.py checks that on the CPU).  reg_loss: rtol 1e-4, as
there (float32 sums of up to 2 M squares in an order the atomics leave free).  Everything else is exact: the bf16 copy, a clip
scale of 1.0f, a gated launch, a frozen range, the step count, the two access paths.

Sizes: those of test_gpu_grad_clip.py -- 1; 3 (tail only); 4 * 64 + 3 aligned and with every pointer one float behind a 16-byte
boundary (the element-by-element path); 100003 (many workgroups and a tail); one full grid stride of 16-byte groups plus
4 * 64 + 3, the stride read from the library (the optimiser's launch and the norm's share grid_for and its cap).

Trainer level.  Two runs of one training step need not agree to the bit (the backward pass adds with float atomics, as
test_gpu_grad_clip.py notes), so wherever bytes are compared the optimiser phase runs twice on ONE set of gradients.
"""
import numpy as np
import pytest

from tests import clip_oracle as CO
from tests import test_gpu_grad_clip as GC
from tests import test_optimizer_cpu as OC

pytestmark = pytest.mark.gpu

RTOL, ATOL, WD, HY = OC.RTOL, OC.ATOL, OC.KERNEL_WD, OC.KERNEL_HYPER
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)
N_SIZES = 6
NAMES = ("w", "a", "b", "ema", "wb", "reg_loss")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from multibox_amd import _lib
    return torch, _lib.lib()


def sizes(l):
    s = GC.sizes(l)[:N_SIZES]
    assert [n for n, off in s if off == 0] == list(OC.KERNEL_NS), "test_optimizer_cpu.KERNEL_NS must name the sizes used here"
    return s


def seed_of(n):
    return 300 + OC.KERNEL_NS.index(n)                        # the seeds test_optimizer_cpu.py checked


def close(got, want):
    """got (device float32) against want (float64 numpy) at the bar; returns the worst error in units of the bar."""
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / (ATOL + RTOL * np.abs(want))
    return float(err.max())


class State:
    """w, g, the two slots, ema, wb, reg of one flat range on the device, every pointer `off` floats behind a 16-byte boundary."""

    def __init__(self, torch, w, g, ema, off=0, a=None, b=None):
        n = len(w)
        z = np.zeros(n, np.float32)
        self.n, self.w, self.g, self.ema = n, GC.dev(torch, w, off), GC.dev(torch, g, off), GC.dev(torch, ema, off)
        self.a, self.b = GC.dev(torch, z if a is None else a, off), GC.dev(torch, z if b is None else b, off)
        self.wb = torch.zeros(n + 2 * off, dtype=torch.bfloat16, device="cuda")[2 * off:]
        self.reg = torch.zeros(1, dtype=torch.float32, device="cuda")

    def tensors(self):
        return (self.w, self.a, self.b, self.ema, self.wb, self.reg)

    def snapshot(self):
        return [t.clone() for t in self.tensors()]

    def step(self, l, rule, kw, wd=WD, ctl=None, clipped=0, trainable=1, calls=0, skipped=None, lr=HY["lr"]):
        from multibox_amd import _lib
        p = lambda t: None if t is None else t.data_ptr()
        if rule == "sgd":
            st = l.mbx_sgd_ema_step(p(self.w), p(self.g), p(self.a) if kw["momentum"] else None, p(self.ema), p(self.wb), self.n, lr,
                                    kw["momentum"], int(kw["nesterov"]), wd, HY["d"], trainable, p(self.reg), p(ctl), clipped, GC.S())
        else:
            st = l.mbx_adam_ema_step(p(self.w), p(self.g), p(self.a), p(self.b), p(self.ema), p(self.wb), self.n, lr, ADAM["beta1"],
                                     ADAM["beta2"], ADAM["eps"], wd, kw["wd_decoupled"], calls, p(skipped), HY["d"], trainable,
                                     p(self.reg), p(ctl), clipped, GC.S())
        _lib.check(st, rule)


def slots_of(rule, kw):
    """Which of the slots (a, b) the rule keeps."""
    return (rule == "adam" or bool(kw["momentum"]), rule == "adam")


def clip_block(torch, scale, ctl=(0.0, 0.0)):
    return torch.tensor([ctl[0], ctl[1], scale, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")


def check_against_oracle(torch, l, n, off, rule, kw, scale=None):
    w, g, ema = OC.kernel_data(n, seed_of(n))
    st = State(torch, w, g, ema, off)
    clip = None if scale is None else clip_block(torch, scale)
    want = OC.two_steps(np.float64, w, g, ema, rule, kw, scale=scale)
    has_a, has_b = slots_of(rule, kw)
    w_before = w.astype(np.float64)
    for k, (ww, wa, wbb, wema) in enumerate(want):
        st.reg.zero_()
        st.step(l, rule, kw, ctl=clip, clipped=int(clip is not None), calls=k)
        errs = dict(w=close(st.w, ww), ema=close(st.ema, wema))
        if has_a:
            errs["a"] = close(st.a, wa)
        if has_b:
            errs["b"] = close(st.b, wbb)
        print("n=%d off=%d %s %r scale=%r step %d: worst errors (x bar) %s" % (n, off, rule, kw, scale, k + 1, errs))
        assert max(errs.values()) <= 1.0, errs
        if not has_a:
            assert not st.a.any()                             # a slot the rule does not keep is never touched
        if not has_b:
            assert not st.b.any()
        reg_ref = 0.5 * OC.f32(WD) * float((w_before ** 2).sum())
        assert np.isclose(float(st.reg), reg_ref, rtol=1e-4), (float(st.reg), reg_ref)
        assert torch.equal(st.wb.float(), st.w.to(torch.bfloat16).float())
        w_before = st.w.cpu().numpy().astype(np.float64)
    assert np.abs(want[1][0] - w.astype(np.float64)).max() > 1e-3          # the two steps moved the weights
    return st, want


# ------------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("case", range(N_SIZES))
@pytest.mark.parametrize("rule,kw", OC.RULES)
def test_two_steps_against_the_oracle(gpu, case, rule, kw):
    torch, l = gpu
    n, off = sizes(l)[case]
    check_against_oracle(torch, l, n, off, rule, kw)


CLIP_RULES = [OC.RULES[0], OC.RULES[1], OC.RULES[3], OC.RULES[5]]          # sgd plain / momentum / nesterov, adamw


@pytest.mark.parametrize("case", range(N_SIZES))
@pytest.mark.parametrize("rule,kw", CLIP_RULES)
def test_scale_half_is_the_oracle_on_half_the_gradient(gpu, case, rule, kw):
    torch, l = gpu
    n, off = sizes(l)[case]
    st, want = check_against_oracle(torch, l, n, off, rule, kw, scale=0.5)
    # the unscaled result differs: the scale was used (Adam's weights hardly show it -- its step is scale-free -- its moments do)
    w, g, ema = OC.kernel_data(n, seed_of(n))
    plain = OC.two_steps(np.float64, w, g, ema, rule, kw)[1]
    got, other = (st.a, plain[1]) if slots_of(rule, kw)[0] else (st.w, plain[0])
    assert not np.allclose(got.cpu().numpy(), other, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("case", range(N_SIZES))
@pytest.mark.parametrize("rule,kw", CLIP_RULES)
def test_scale_one_is_byte_identical_to_the_unclipped_step(gpu, case, rule, kw):
    """reg_loss is summed over workgroups with float atomics, whose order is free: the weights are small integers and the
    decay a power of two, so every partial sum of w^2 is exact and its bytes do not depend on that order (as in
    test_gpu_grad_clip.py).  After the first step the weights are arbitrary reals: reg_loss is left out of the second."""
    torch, l = gpu
    n, off = sizes(l)[case]
    rng = np.random.RandomState(400 + case)
    w, g = rng.randint(-2, 3, n).astype(np.float32), (rng.randn(n) * 10).astype(np.float32)
    wd = 2.0 ** -14
    plain, clipped = State(torch, w, g, w * 0.5, off), State(torch, w, g, w * 0.5, off)
    clip = clip_block(torch, 1.0)
    assert clip[2:3].cpu().numpy().tobytes() == GC.ONE_BITS
    for k in range(2):
        plain.step(l, rule, kw, wd=wd, calls=k)
        clipped.step(l, rule, kw, wd=wd, ctl=clip, clipped=1, calls=k)
        for name, a, b in zip(NAMES[:5] if k else NAMES, plain.tensors(), clipped.tensors()):
            assert GC.same_bits(torch, a, b), (name, k)
        if k == 0:
            assert float(plain.reg) == 0.5 * wd * float((w.astype(np.float64) ** 2).sum())
            assert not torch.equal(plain.w, GC.dev(torch, w, off))


# ------------------------------------------------------------------------------------------------------ gate, frozen ranges
BOTH = [OC.RULES[3], OC.RULES[5]]                              # sgd with momentum and nesterov; adamw


@pytest.mark.parametrize("rule,kw", BOTH)
@pytest.mark.parametrize("ctl", [(1.0, 0.0), (0.0, 2.0)])
@pytest.mark.parametrize("clipped", [0, 1])
def test_flagged_control_block_changes_nothing(gpu, rule, kw, ctl, clipped):
    torch, l = gpu
    for n, off in ((259, 0), (259, 1)):
        w, g, ema = OC.kernel_data(n, 7)
        st = State(torch, w, g, ema, off, a=g * 0.25, b=g * g)
        block = clip_block(torch, 0.5, ctl)
        before = st.snapshot()
        st.step(l, rule, kw, ctl=block, clipped=clipped)
        torch.cuda.synchronize()
        for name, a, b in zip(NAMES, before, st.tensors()):
            assert GC.same_bits(torch, a, b), (name, n, off)
        assert block[:3].tolist() == [ctl[0], ctl[1], 0.5]    # the block is only read
    # the same launch with a clear block applies the step
    st.step(l, rule, kw, ctl=clip_block(torch, 0.5), clipped=clipped)
    assert not torch.equal(st.w, before[0]) and float(st.reg) > 0


@pytest.mark.parametrize("rule,kw", BOTH)
def test_frozen_range_gets_ema_regulariser_and_bf16_only(gpu, rule, kw):
    torch, l = gpu
    for n, off in ((259, 0), (259, 1), (100003, 0)):
        w, g, ema = OC.kernel_data(n, 8)
        st = State(torch, w, g, ema, off, a=g * 0.25, b=g * g)
        before = st.snapshot()
        st.step(l, rule, kw, trainable=0, calls=3)
        for name, a, b in zip(NAMES[:3], before, st.tensors()):
            assert GC.same_bits(torch, a, b), (name, n, off)
        assert close(st.ema, OC.ema_step(ema.astype(np.float64), w.astype(np.float64), HY["d"])) <= 1.0
        assert np.isclose(float(st.reg), 0.5 * OC.f32(WD) * float((w.astype(np.float64) ** 2).sum()), rtol=1e-4)
        assert torch.equal(st.wb.float(), st.w.to(torch.bfloat16).float()) and bool(st.wb.any())


# ------------------------------------------------------------------------------------------------------ Adam's step count
def test_skipped_steps_come_off_the_step_count(gpu):
    torch, l = gpu
    rule, kw = OC.RULES[5]
    w, g, ema = OC.kernel_data(100003, 9)
    a, b = g * 0.25, g * g * 0.5
    with_counter, plain, wrong = (State(torch, w, g, ema, a=a, b=b) for _ in range(3))
    skipped = torch.tensor([2], dtype=torch.int64, device="cuda")
    with_counter.step(l, rule, kw, calls=5, skipped=skipped)
    plain.step(l, rule, kw, calls=3)
    wrong.step(l, rule, kw, calls=5)
    assert skipped.tolist() == [2]                            # only read
    for name, x, y in zip(NAMES[:5], with_counter.tensors(), plain.tensors()):
        assert GC.same_bits(torch, x, y), name
    assert not torch.equal(wrong.w, plain.w)                  # (t = 6 instead of 4 is another step)


def test_first_step_from_zero_moments_moves_every_weight_by_lr(gpu):
    """t = 1: m^ = g', v^ = g'^2, so |dw| = lr * |g'| / (|g'| + eps) = lr to 2e-8 (|g'| >= 0.5).  The old weight is exact
    and the new one is rounded once: half an ulp of a value below 2.01 is 1.2e-7; the bound is 2e-7."""
    torch, l = gpu
    rule, kw = OC.RULES[4]
    for n, off in ((259, 1), (100003, 0)):
        w, g, ema = OC.kernel_data(n, 10)
        st = State(torch, w, g, ema, off)
        st.step(l, rule, kw, wd=0.0, calls=0)
        dw = st.w.cpu().numpy().astype(np.float64) - w
        assert np.abs(np.abs(dw) - OC.f32(HY["lr"])).max() < 2e-7 and (np.sign(dw) == -np.sign(g)).all()
        late = State(torch, w, g, ema, off)                   # the same launch taken for step 11: no such step
        late.step(l, rule, kw, wd=0.0, calls=10)
        dl = np.abs(late.w.cpu().numpy().astype(np.float64) - w)
        assert (dl < 0.6 * HY["lr"]).all() and (dl > 0.3 * HY["lr"]).all()


# ------------------------------------------------------------------------------------------------------ the two access paths
@pytest.mark.parametrize("rule,kw", [OC.RULES[0], OC.RULES[3], OC.RULES[5]])
@pytest.mark.parametrize("clipped", [0, 1])
def test_vector_and_element_paths_agree_to_the_bit(gpu, rule, kw, clipped):
    """The same values at offset 0 (16-byte accesses and a tail of 3) and at offset 1 (element by element).  reg_loss is left
    out: the two paths deal the elements to other lanes, so its float32 partial sums differ."""
    torch, l = gpu
    for n in (259, 100003):
        w, g, ema = OC.kernel_data(n, 11)
        vec, elem = State(torch, w, g, ema, 0), State(torch, w, g, ema, 1)
        assert vec.w.data_ptr() % 16 == 0 and elem.w.data_ptr() % 16 == 4
        clip = clip_block(torch, 0.7) if clipped else None
        for k in range(2):
            for st in (vec, elem):
                st.step(l, rule, kw, ctl=clip, clipped=clipped, calls=k)
            for name, a, b in zip(NAMES[:5], vec.tensors(), elem.tensors()):
                assert GC.same_bits(torch, a, b), (name, n, k)
        assert not torch.equal(vec.w, GC.dev(torch, w))


# ------------------------------------------------------------------------------------------------------ through the Trainer
# (sgd: this loss is a batch sum weighted by LOCATION_LOSS_ALPHA = 1000 and its gradients are of order 100; plain SGD at the
# reference's learning rate of 0.01, sized for RMSProp's normalised step, leaves the finite range in one step)
TRAINER_RULES = {"sgd": dict(optimizer="sgd", sgd_momentum=0.9, sgd_nesterov=True, initial_learning_rate=1e-5),
                 "adam": dict(optimizer="adam"),
                 "adamw": dict(optimizer="adamw", adamw_weight_decay=0.01)}


def oracle_step(torch, tr, name, t, p, g, a, b, wd, wdd):
    """One oracle step of the trainer's rule on float64 device tensors; (p, a, b)."""
    if name == "sgd":
        p, a = OC.sgd_step(p, g, a, tr.lr, momentum=tr.sgd_momentum, nesterov=tr.sgd_nesterov, wd=wd)
        return p, a, b
    return OC.adam_step(p, g, a, b, t, tr.lr, beta1=tr.adam_beta1, beta2=tr.adam_beta2, eps=tr.adam_eps, wd=wd, wd_decoupled=wdd)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("name", sorted(TRAINER_RULES))
def test_trainer_two_steps_against_the_oracle(gpu, name, use_graph):
    torch, l = gpu
    from multibox_amd.engine import WEIGHT_DECAY
    net, tr = GC.make_trainer(torch, use_graph, **TRAINER_RULES[name])
    assert tr.opt_ranges == [("W", 0, net.nW, 1), ("Bt", 0, net.nBt, 1)]
    assert (tr.Wms is None) == (name == "sgd") and tr.Wmom is not None and not tr.Wmom.any()
    assert name == "sgd" or not tr.Wms.any()
    wd, wdd = (0.0, 0.01) if name == "adamw" else (WEIGHT_DECAY, 0.0)
    W0, Bt0 = net.W.clone(), net.Bt.clone()
    ref = {"W": [net.W.double(), 0.0, 0.0], "Bt": [net.Bt.double(), 0.0, 0.0]}
    for t in (1, 2):
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0 and int(tr.skipped_steps) == 0
        for key, g, c, cd in (("W", net.Wg, wd, wdd), ("Bt", net.Btg[:net.nBt], 0.0, 0.0)):
            ref[key] = list(oracle_step(torch, tr, name, t, ref[key][0], g.double(), ref[key][1], ref[key][2], c, cd))
        loc, conf, reg, total = tr.losses()
        if name == "adamw":
            assert reg == 0.0 and total == loc + conf
        else:
            assert reg > 0.0
    # The first slot is a sum of two terms of the size of the gradient that may cancel (the second step's gradient against the
    # first's): each term is rounded relative to ITSELF, so its bar is relative to |slot| + |g|, not to |slot| alone.
    for key, now, p0, slot, g in (("W", net.W, W0, tr.Wmom, net.Wg), ("Bt", net.Bt, Bt0, tr.Btmom, net.Btg[:net.nBt])):
        want = ref[key][0]
        err = ((now.double() - want).abs() / (ATOL + RTOL * want.abs())).max().item()
        moved = (want - p0.double()).abs().max().item()
        serr = ((slot.double() - ref[key][1]).abs() / (ATOL + RTOL * (ref[key][1].abs() + g.double().abs()))).max().item()
        print("%s graph=%d %s: worst error %.3g x bar (first slot %.3g x bar), largest update %.3g, largest gradient %.3g" % (
            name, use_graph, key, err, serr, moved, g.abs().max().item()))
        assert err <= 1.0 and serr <= 1.0, key
        assert moved > (10 * ATOL if key == "W" else ATOL), key       # the comparison is of updates, not of untouched weights
    assert tr.global_step == 2 and tr.optimizer_steps() == 2


class Recorder(GC.Recorder):
    """GC.Recorder that also keeps the arguments of mbx_grad_sqnorm."""

    def __init__(self, lib):
        super().__init__(lib)
        self.sqnorm_args = []

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if name != "mbx_grad_sqnorm":
            return fn

        def wrapped(*a):
            self.sqnorm_args.append(a)
            return fn(*a)
        return wrapped


def test_adamw_clips_the_norm_of_the_gradient_alone(gpu):
    torch, l = gpu
    from multibox_amd import _lib
    rec = Recorder(l)
    _lib._lib = rec
    try:
        net, tr = GC.make_trainer(torch, False, clip_gradient_norm=float("inf"), **TRAINER_RULES["adamw"])
        tr.step()
        torch.cuda.synchronize()
    finally:
        _lib._lib = l
    Wg, Btg = net.Wg.cpu().numpy(), net.Btg.cpu().numpy()[:net.nBt]
    want = CO.global_norm([(Wg, None, 0.0), (Btg, None, 0.0)])
    print("adamw: grad_norm %r, oracle on g alone %r" % (tr.grad_norm(), want))
    assert np.isfinite(want) and want > 0 and np.isclose(tr.grad_norm(), want, rtol=1e-6, atol=0)
    assert [(a[1], a[3]) for a in rec.sqnorm_args] == [(None, 0.0), (None, 0.0)]          # w = NULL, wd = 0 for both ranges
    assert rec.names.count("mbx_adam_ema_step") == 2 and "mbx_rmsprop_ema_step_clipped" not in rec.names
    assert tr.clip_scale() == 1.0 and tr.losses()[2] == 0.0


def parent_optimizer_phase(torch, tr):
    """The optimiser phase as it was before OPTIMIZER existed, call for call (no clipping, momentum 0)."""
    from multibox_amd import _lib
    from multibox_amd.engine import WEIGHT_DECAY
    from multibox_amd.trainer import learning_rate
    net, l = tr.net, _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    t = tr.global_step
    lr = learning_rate(t, tr.lr0, tr.dsteps, tr.lr_factor, tr.staircase)
    d = min(tr.ema_decay, (1.0 + t) / (10.0 + t))
    ctl = net.step_ctl.data_ptr()
    _lib.check(l.mbx_rmsprop_ema_step(net.W.data_ptr(), net.Wg.data_ptr(), tr.Wms.data_ptr(), None, tr.Wema.data_ptr(), net.Wb.data_ptr(),
                                      net.nW, lr, tr.rms_decay, tr.momentum, tr.eps, WEIGHT_DECAY, d, 1, net.reg_loss.data_ptr(), ctl, s), "W")
    _lib.check(l.mbx_rmsprop_ema_step(net.Bt.data_ptr(), net.Btg.data_ptr(), tr.Btms.data_ptr(), None, tr.Btema.data_ptr(), None,
                                      net.nBt, lr, tr.rms_decay, tr.momentum, tr.eps, 0.0, d, 1, None, ctl, s), "beta")
    net.apply_moving_update(net.step_ctl, tr.skipped_steps, tr.MMema, tr.MVema, d)
    net.prepare_filters()


def state_of(net, tr):
    ts = dict(W=net.W, Bt=net.Bt, Wb=net.Wb, Wms=tr.Wms, Btms=tr.Btms, Wmom=tr.Wmom, Btmom=tr.Btmom, Wema=tr.Wema, Btema=tr.Btema,
              MM=net.MM, MV=net.MV, MMema=tr.MMema, MVema=tr.MVema)
    return {k: v for k, v in ts.items() if v is not None}


def test_trainer_without_the_key_is_the_parent_step(gpu):
    """The second step's optimiser phase twice on one set of gradients: through the Trainer, and as the calls the phase consisted
    of before -- every parameter, slot and shadow has the same bytes.  Neither step asks the library for a new entry point."""
    torch, l = gpu
    from multibox_amd import _lib
    rec = GC.Recorder(l)
    _lib._lib = rec
    try:
        net, tr = GC.make_trainer(torch, False)
        assert tr.optimizer == "rmsprop" and tr.Wmom is None and bool((tr.Wms == 1).all()) and tr.warmup_steps == 0
        tr.step()
        tr.run_eager_once()                                   # forward + loss + backward of step 2; the optimiser follows by hand
        torch.cuda.synchronize()
        live = state_of(net, tr)
        before = {k: v.clone() for k, v in live.items()}
        tr._optimizer()
        torch.cuda.synchronize()
        ours = {k: v.clone() for k, v in live.items()}
        lr_ours = tr.lr
        for k, v in live.items():
            v.copy_(before[k])
        parent_optimizer_phase(torch, tr)
        torch.cuda.synchronize()
    finally:
        _lib._lib = l
    for k, v in live.items():
        assert GC.same_bits(torch, v, ours[k]), k
    assert not torch.equal(ours["W"], before["W"]) and not torch.equal(ours["Wms"], before["Wms"])
    from multibox_amd.trainer import learning_rate
    assert lr_ours == learning_rate(1, tr.lr0, tr.dsteps, tr.lr_factor, tr.staircase)
    assert not {"mbx_sgd_ema_step", "mbx_adam_ema_step"} & set(rec.names)
    assert rec.names.count("mbx_rmsprop_ema_step") == 6       # two ranges, three optimiser phases


def test_warmup_scales_the_learning_rate_of_the_step(gpu):
    torch, l = gpu
    from multibox_amd.trainer import learning_rate
    net, tr = GC.make_trainer(torch, False, lr_warmup_steps=4, **TRAINER_RULES["sgd"])
    base = learning_rate(0, tr.lr0, tr.dsteps, tr.lr_factor, tr.staircase)
    tr.run_eager_once()
    for t, factor in ((0, 0.25), (2, 0.75), (3, 1.0), (9, 1.0)):
        tr.global_step = t
        tr._optimizer()
        assert tr.lr == base * factor, t
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ checkpoint
CKPT_COMPARED = ("W", "Bt", "Wb", "Wms", "Btms", "Wmom", "Btmom", "Wema", "Btema")


@pytest.mark.parametrize("name", ["rmsprop", "sgd", "adam", "adamw"])
def test_checkpoint_resumes_to_the_same_bytes(gpu, tmp_path, name):
    """Save after one step, restore into a fresh Trainer, apply the second step's optimiser phase to the gradients the first
    Trainer computed for it (module docstring): parameters, slots and shadows equal the uninterrupted run's to the bit -- the
    slots, the step count of Adam's bias correction and the schedule's global_step all came through the file.  (The moving
    statistics are left out: the fresh Trainer has not seen the batch.)"""
    torch, l = gpu
    from multibox_amd import checkpoint as CK
    kw = TRAINER_RULES.get(name, {})
    net, tr = GC.make_trainer(torch, False, **kw)
    tr.step()
    torch.cuda.synchronize()
    path = CK.save(str(tmp_path), tr)
    st = torch.load(path, map_location="cpu")
    assert st["optimizer"] == name and st["global_step"] == 1 and st["opt_steps"] == 1
    assert ("Wms" in st) == (name != "sgd") and ("Wmom" in st) == (name != "rmsprop")
    tr.run_eager_once()
    torch.cuda.synchronize()
    grads = net.G.clone()
    tr._optimizer()
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in state_of(net, tr).items() if k in CKPT_COMPARED}
    w_saved = st["W"]
    del st, tr, net
    torch.cuda.empty_cache()
    net2, tr2 = GC.make_trainer(torch, False, **kw)
    CK.restore_for_training(path, tr2)
    assert tr2.global_step == 1 and tr2.optimizer_steps() == 1 and not tr2.events
    assert torch.equal(net2.W.cpu(), w_saved)
    net2.zero_grads()
    net2.G.copy_(grads)
    tr2._optimizer()
    torch.cuda.synchronize()
    got = state_of(net2, tr2)
    assert sorted(k for k in got if k in CKPT_COMPARED) == sorted(want)
    for k, v in want.items():
        assert GC.same_bits(torch, got[k], v), k
    assert not torch.equal(net2.W.cpu(), w_saved)
    # the same file as --pretrained_model under the same rule: the schedule starts over, the slots keep their step count
    CK.restore_pretrained(path, tr2)
    assert tr2.global_step == 0 and tr2.optimizer_steps() == 1 and not tr2.events and torch.equal(net2.W.cpu(), w_saved)
    net2.G.copy_(grads)
    tr2._optimizer()                                          # (Adam: step 2 of its slots at global_step 0)
    tr2.global_step += 1
    torch.cuda.synchronize()
    assert tr2.optimizer_steps() == 2 and bool(torch.isfinite(net2.W).all())
    if name != "rmsprop":
        return
    # an rmsprop checkpoint under adam: variables, shadows and global_step are restored, the moments stay zero, the log hears of it
    del tr2, net2, got
    torch.cuda.empty_cache()
    net3, tr3 = GC.make_trainer(torch, False, **TRAINER_RULES["adam"])
    assert not torch.equal(net3.W.cpu(), w_saved)
    CK.restore_for_training(path, tr3)
    assert torch.equal(net3.W.cpu(), w_saved) and torch.equal(tr3.Wema.cpu(), torch.load(path, map_location="cpu")["Wema"])
    assert tr3.global_step == 1 and tr3.optimizer_steps() == 0
    assert not tr3.Wmom.any() and not tr3.Wms.any() and not tr3.Btmom.any() and not tr3.Btms.any()
    assert tr3.events[-1]["event"] == "optimizer_changed" and tr3.events[-1]["checkpoint_optimizer"] == "rmsprop"
    assert tr3.events[-1]["optimizer"] == "adam" and tr3.events[-1]["global_step"] == 1
    # ... and as --pretrained_model under adam: global_step 0, no step on the fresh moments yet, and the first step is Adam's
    # step 1 -- every weight with a gradient moves by lr (step 2 from zero moments would move it by 0.74 lr)
    CK.restore_pretrained(path, tr3)
    assert tr3.global_step == 0 and tr3.optimizer_steps() == 0 and torch.equal(net3.W.cpu(), w_saved)
    assert not tr3.Wmom.any() and not tr3.Wms.any() and tr3.events[-1]["event"] == "optimizer_changed"
    tr3.step()
    torch.cuda.synchronize()
    assert tr3.global_step == 1 and tr3.optimizer_steps() == 1 and int(tr3.skipped_steps) == 0
    dw = (net3.W.cpu().double() - w_saved.double()).abs()
    big = net3.Wg.cpu().abs() > 1e-3                          # (|g'| >> eps = 1e-8; WEIGHT_DECAY * w is at most 1e-5 beside it)
    assert int(big.sum()) > 1000 and float((dw[big] - tr3.lr).abs().max()) < 1e-3 * tr3.lr + 2e-7
    path2 = CK.save(str(tmp_path), tr3)
    assert torch.load(path2, map_location="cpu")["opt_steps"] == 1
