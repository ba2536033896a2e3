"""GPU: layer-wise trust ratios (mbx_trust_norms_sgd, mbx_trust_moments_adam, mbx_trust_ratios, mbx_sgd_ema_step_trust,
mbx_adam_ema_step_trust, Trainer(layerwise_trust=True)) against the oracles of tests/trust_oracle.py.

Bars (tests/test_trust_cpu.py derives them and checks that a float32 restatement alone meets them on this very data).
Ratios: rtol 1e-6.  Updates: rtol 1e-5 / atol 1e-6 on w, the slots and ema; wb is bf16(w) exactly; reg_loss rtol 1e-4 (float32
sums in an order the atomics leave free).  Everything else is exact: a ratio of 1.0f, a gated launch, a repeated launch.

The partition is trust_oracle.SMALL (chunk size read from the library), once with every pointer 16-byte aligned and once with
every pointer one float behind a boundary (the element-by-element path).

Trainer level.  Two runs of one training step need not agree to the bit (the backward pass adds with float atomics), so wherever
bytes are compared the optimiser phase runs on ONE set of gradients.
"""
import ctypes as C
import re

import numpy as np
import pytest

from tests import test_gpu_grad_clip as GC
from tests import test_gpu_optimizer as GO
from tests import test_optimizer_cpu as OC
from tests import trust_oracle as TO

pytestmark = pytest.mark.gpu

RTOL, ATOL, WD, HY, ADAM = OC.RTOL, OC.ATOL, OC.KERNEL_WD, OC.KERNEL_HYPER, GO.ADAM
RATIO_RTOL = 1e-6
NAMES = ("w", "a", "b", "ema", "wb")
TRUST_ENTRIES = {"mbx_trust_chunk_elems", "mbx_trust_plan_count", "mbx_trust_plan", "mbx_trust_norms_sgd", "mbx_trust_moments_adam",
                 "mbx_trust_ratios", "mbx_sgd_ema_step_trust", "mbx_adam_ema_step_trust"}


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from multibox_amd import _lib
    return torch, _lib.lib()


class Plan:
    """The uploaded plan of one partition with its partial sums and ratios (filled with values no launch writes)."""

    def __init__(self, torch, l, bounds, adapt):
        from multibox_amd import _lib
        nv = len(bounds) - 1
        b = (C.c_int64 * (nv + 1))(*[int(x) for x in bounds])
        a = (C.c_int32 * nv)(*[int(x) for x in adapt])
        nc = int(l.mbx_trust_plan_count(b, nv))
        chunks, vars_ = (_lib.TrustChunk * nc)(), (_lib.TrustVar * nv)()
        _lib.check(l.mbx_trust_plan(b, a, nv, chunks, vars_), "plan")
        up = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
        self.bounds, self.adapt, self.nv, self.nc = np.asarray(bounds), list(adapt), nv, nc
        self.host_chunks = np.frombuffer(bytes(chunks), TO.CHUNK_DTYPE)
        self.chunks, self.vars = up(chunks), up(vars_)
        self.partials = torch.full((2 * nc,), -3.0, dtype=torch.float64, device="cuda")
        self.ratio = torch.full((nv,), -7.0, dtype=torch.float32, device="cuda")


class State(GO.State):
    """test_gpu_optimizer.State with a plan: step() is the twin's launch, trust_step() the three trusted ones."""

    def __init__(self, torch, l, w, g, ema, bounds, adapt, off=0, a=None, b=None):
        super().__init__(torch, w, g, ema, off, a, b)
        self.plan = Plan(torch, l, bounds, adapt)

    def norms(self, l, rule, kw, coeff=TO.COEFF, wd=WD, ctl=None, clipped=0, calls=0):
        from multibox_amd import _lib
        p = lambda t: None if t is None else t.data_ptr()
        pl = self.plan
        if rule == "sgd":
            st = l.mbx_trust_norms_sgd(p(self.w), p(self.g), p(pl.chunks), pl.nc, wd, p(pl.partials), p(ctl), clipped, GC.S())
        else:
            st = l.mbx_trust_moments_adam(p(self.w), p(self.g), p(self.a), p(self.b), p(pl.chunks), pl.nc, ADAM["beta1"], ADAM["beta2"],
                                          ADAM["eps"], wd, kw["wd_decoupled"], calls, None, p(pl.partials), p(ctl), clipped, GC.S())
        _lib.check(st, rule + " norms")
        _lib.check(l.mbx_trust_ratios(p(pl.partials), p(pl.vars), pl.nv, coeff, p(pl.ratio), p(ctl), GC.S()), "ratios")

    def apply(self, l, rule, kw, wd=WD, ctl=None, clipped=0, calls=0, lr=HY["lr"], trainable=1):
        from multibox_amd import _lib
        p = lambda t: None if t is None else t.data_ptr()
        pl = self.plan
        tail = (p(pl.chunks), pl.nc, p(pl.ratio), GC.S())
        if rule == "sgd":
            st = l.mbx_sgd_ema_step_trust(p(self.w), p(self.g), p(self.a) if kw["momentum"] else None, p(self.ema), p(self.wb), self.n, lr,
                                          kw["momentum"], int(kw["nesterov"]), wd, HY["d"], trainable, p(self.reg), p(ctl), clipped, *tail)
        else:
            st = l.mbx_adam_ema_step_trust(p(self.w), p(self.g), p(self.a), p(self.b), p(self.ema), p(self.wb), self.n, lr, ADAM["beta1"],
                                           ADAM["beta2"], ADAM["eps"], wd, kw["wd_decoupled"], calls, None, HY["d"], trainable, p(self.reg),
                                           p(ctl), clipped, *tail)
        _lib.check(st, rule + " apply")

    def trust_step(self, l, rule, kw, coeff=TO.COEFF, wd=WD, ctl=None, clipped=0, calls=0):
        self.norms(l, rule, kw, coeff, wd, ctl, clipped, calls)
        self.apply(l, rule, kw, wd, ctl, clipped, calls)

    def everything(self):
        return self.tensors() + (self.plan.partials, self.plan.ratio)


def small_state(torch, l, off, adapt=None, **kw):
    CH = int(l.mbx_trust_chunk_elems())
    bounds, ad = TO.small(CH)
    w, g, ema = TO.small_data(CH)
    st = State(torch, l, w, g, ema, bounds, ad if adapt is None else adapt, off, **kw)
    assert st.w.data_ptr() % 16 == 4 * off and st.plan.nc == len(TO.plan(bounds, CH)[0])
    return st, (w, g, ema, bounds, ad)


# ------------------------------------------------------------------------------------------------------ 1. ratios
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rule,kw", [TO.CASES[1], TO.CASES[4], TO.CASES[5]])
def test_ratios_against_the_oracle(gpu, rule, kw, off):
    """With wd = 0.05 every ratio against the oracle (the zero-g variable has x = wd * w there: coeff / wd under sgd); with
    wd = 0 the zero-g variable has x = 0 -- under the Adam rule on its first step with wd_decoupled 0 as well, u = 0 -- and its
    ratio is exactly 1.0f, like the zero-w variable's and the non-adapting ones' in both runs."""
    torch, l = gpu
    for wd, wdd in ((WD, None), (0.0, 0.0)):
        st, (w, g, ema, bounds, adapt) = small_state(torch, l, off)
        k = dict(kw) if wdd is None or rule == "sgd" else dict(kw, wd_decoupled=wdd)
        st.norms(l, rule, k, wd=wd)
        want = TO.two_steps(np.float64, w, g, ema, bounds, adapt, rule, k, wd=wd)[0][4]
        got = st.plan.ratio.cpu().numpy()
        print("%s %r off=%d wd=%g: worst relative error %.3g" % (rule, k, off, wd, np.abs(got / want - 1).max()))
        assert np.allclose(got, want, rtol=RATIO_RTOL, atol=0), (got, want)
        ones = [TO.ZERO_W, len(adapt) - 2, len(adapt) - 1] + ([TO.ZERO_G] if wd == 0.0 else [])
        assert got[ones].tobytes() == GC.ONE_BITS * len(ones)
        assert (got[[i for i in range(len(adapt)) if i not in ones and i != TO.ZERO_G]] != 1.0).all()
        # the slots: per chunk the sum of squares of its own elements
        part = st.plan.partials.cpu().numpy().reshape(-1, 2)
        sums = np.array([float((w[c["lo"]:c["lo"] + c["len"]].astype(np.float64) ** 2).sum()) for c in st.plan.host_chunks])
        assert np.allclose(part[:, 0], sums, rtol=1e-12, atol=0) and (part[:, 1] >= 0).all()


# ------------------------------------------------------------------------------------------------------ 2. updates
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("rule,kw", TO.CASES)
def test_two_steps_against_the_oracle(gpu, rule, kw, off):
    torch, l = gpu
    st, (w, g, ema, bounds, adapt) = small_state(torch, l, off)
    want = TO.two_steps(np.float64, w, g, ema, bounds, adapt, rule, kw)
    has_a, has_b = GO.slots_of(rule, kw)
    w_before = w.astype(np.float64)
    for k, (ww, wa, wbb, wema, wr) in enumerate(want):
        st.reg.zero_()
        st.trust_step(l, rule, kw, calls=k)
        errs = dict(w=GO.close(st.w, ww), ema=GO.close(st.ema, wema))
        if has_a:
            errs["a"] = GO.close(st.a, wa)
        if has_b:
            errs["b"] = GO.close(st.b, wbb)
        r = st.plan.ratio.cpu().numpy()
        print("off=%d %s %r step %d: worst errors (x bar) %s, ratio %.3g" % (off, rule, kw, k + 1, errs, np.abs(r / wr - 1).max()))
        assert max(errs.values()) <= 1.0, errs
        assert np.allclose(r, wr, rtol=RATIO_RTOL, atol=0)
        if not has_a:
            assert not st.a.any()
        if not has_b:
            assert not st.b.any()
        reg_ref = 0.5 * OC.f32(WD) * float((w_before ** 2).sum())
        assert np.isclose(float(st.reg), reg_ref, rtol=1e-4), (float(st.reg), reg_ref)
        assert torch.equal(st.wb.float(), st.w.to(torch.bfloat16).float())
        w_before = st.w.cpu().numpy().astype(np.float64)
    assert np.abs(want[1][0] - w.astype(np.float64)).max() > 1e-3
    # not the plain rule's result: the ratios were used
    plain = OC.two_steps(np.float64, w, g, ema, rule, kw)[1][0]
    assert not np.allclose(st.w.cpu().numpy(), plain, rtol=1e-3, atol=1e-6)


# ------------------------------------------------------------------------------------------------------ 3. byte identity
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("clipped", [0, 1])
@pytest.mark.parametrize("rule,kw", [OC.RULES[0], OC.RULES[3], OC.RULES[4], OC.RULES[5]])
def test_ratio_one_is_byte_identical_to_the_twin(gpu, rule, kw, clipped, off):
    torch, l = gpu
    st, (w, g, ema, bounds, adapt) = small_state(torch, l, off, adapt=[0] * 12)
    twin = GO.State(torch, w, g, ema, off)
    clip = GO.clip_block(torch, 0.7) if clipped else None
    for k in range(2):
        st.reg.zero_()
        twin.reg.zero_()
        st.trust_step(l, rule, kw, ctl=clip, clipped=clipped, calls=k)
        twin.step(l, rule, kw, ctl=clip, clipped=clipped, calls=k)
        assert st.plan.ratio.cpu().numpy().tobytes() == GC.ONE_BITS * 12
        for name, a, b in zip(NAMES, st.tensors(), twin.tensors()):
            assert GC.same_bits(torch, a, b), (name, k)
        assert np.isclose(float(st.reg), float(twin.reg), rtol=1e-4) and float(twin.reg) > 0
    assert not torch.equal(st.w, GC.dev(torch, w, off))


# ------------------------------------------------------------------------------------------------------ 4. determinism, partition
@pytest.mark.parametrize("rule,kw", [TO.CASES[3], TO.CASES[5]])
def test_same_inputs_same_bytes(gpu, rule, kw):
    torch, l = gpu
    for off in (0, 1):
        runs = []
        for _ in range(2):
            st, _ = small_state(torch, l, off)
            st.trust_step(l, rule, kw)
            runs.append([t.clone() for t in st.everything()[:5] + st.everything()[6:]])
        for i, (a, b) in enumerate(zip(*runs)):
            assert GC.same_bits(torch, a.view(torch.int64) if a.dtype == torch.float64 else a,
                                b.view(torch.int64) if b.dtype == torch.float64 else b), (i, off)


@pytest.mark.parametrize("rule,kw", [TO.CASES[1], TO.CASES[5]])
def test_ratio_does_not_depend_on_the_neighbours_cut(gpu, rule, kw):
    """One variable of CH + 300 elements at offset 5 of two partitions: [5 | X | 9] and [2, 3 | X | 4, 5].  Its own chunks are the
    same in both, so its slots and its ratio have the same bytes."""
    torch, l = gpu
    CH = int(l.mbx_trust_chunk_elems())
    n = 5 + CH + 300 + 9
    w, g, ema = OC.kernel_data(n, 501)
    got = []
    for lengths, x in (([5, CH + 300, 9], 1), ([2, 3, CH + 300, 4, 5], 2)):
        st = State(torch, l, w, g, ema, TO.bounds_of(lengths), [1] * len(lengths))
        st.norms(l, rule, kw)
        own = st.plan.host_chunks["var"] == x
        assert own.sum() == 2 and st.plan.host_chunks["lo"][own].tolist() == [5, CH]
        part = st.plan.partials.cpu().numpy().reshape(-1, 2)[own]
        got.append((part.tobytes(), st.plan.ratio.cpu().numpy()[x].tobytes()))
    assert got[0] == got[1]


# ------------------------------------------------------------------------------------------------------ 5. gate
@pytest.mark.parametrize("rule,kw", [TO.CASES[3], TO.CASES[5]])
@pytest.mark.parametrize("ctl", [(1.0, 0.0), (0.0, 2.0)])
@pytest.mark.parametrize("clipped", [0, 1])
def test_flagged_block_changes_nothing(gpu, rule, kw, ctl, clipped):
    """clipped = 0: the step control block; clipped = 1: a clip block whose word 1 (or 0) is set."""
    torch, l = gpu
    as_int = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for off in (0, 1):
        CH = int(l.mbx_trust_chunk_elems())
        g0 = TO.small_data(CH)[1]
        st, _ = small_state(torch, l, off, a=g0 * 0.25, b=g0 * g0)
        block = GO.clip_block(torch, 0.5, ctl)
        before = [t.clone() for t in st.everything()]
        st.trust_step(l, rule, kw, ctl=block, clipped=clipped)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(before, st.everything())):
            assert GC.same_bits(torch, as_int(a), as_int(b)), (i, off)
        assert block[:3].tolist() == [ctl[0], ctl[1], 0.5]
    st.trust_step(l, rule, kw, ctl=GO.clip_block(torch, 0.5), clipped=clipped)      # a clear block applies the step
    assert not torch.equal(st.w, before[0]) and float(st.reg) > 0 and float(st.plan.ratio[4]) > 0


# ------------------------------------------------------------------------------------------------------ 6. clip composition
@pytest.mark.parametrize("off", [0, 1])
def test_half_the_gradient_doubles_the_lars_ratio(gpu, off):
    torch, l = gpu
    rule, kw = TO.CASES[1]
    plain, _ = small_state(torch, l, off)
    half, (w, g, ema, bounds, adapt) = small_state(torch, l, off)
    plain.norms(l, rule, kw)
    half.norms(l, rule, kw, ctl=GO.clip_block(torch, 0.5), clipped=1)
    r1, r2 = plain.plan.ratio.cpu().numpy(), half.plan.ratio.cpu().numpy()
    moving = [i for i in range(len(adapt)) if adapt[i] and i != TO.ZERO_W]
    assert np.allclose(r2[moving], 2 * r1[moving], rtol=RATIO_RTOL, atol=0)
    assert (r2[[TO.ZERO_W, -2, -1]] == 1.0).all()
    want = TO.two_steps(np.float64, w, g, ema, bounds, adapt, rule, kw, scale=0.5)[0]
    half.apply(l, rule, kw, ctl=GO.clip_block(torch, 0.5), clipped=1)
    assert np.allclose(r2, want[4], rtol=RATIO_RTOL, atol=0) and GO.close(half.w, want[0]) <= 1.0


# ------------------------------------------------------------------------------------------------------ 7. through the Trainer
# coeff 1 at the default learning rate of 0.01: every filter moves by about 1 % of its norm, far over the bar's atol
TRAINER = {"sgd": dict(optimizer="sgd", sgd_momentum=0.9, sgd_nesterov=True, layerwise_trust=True, trust_coeff=1.0),
           "adamw": dict(optimizer="adamw", adamw_weight_decay=0.01, layerwise_trust=True, trust_coeff=1.0)}


def without_trust(kw):
    return {k: v for k, v in kw.items() if k not in ("layerwise_trust", "trust_coeff")}


def w_variables(net, lo=0):
    """[(name, off, end, adapts)] of the variables in W from lo on, in buffer order; each owns up to the next one's start."""
    ents = sorted((off, n, len(shape) > 1) for n, (buf, off, shape, _) in net.param_index.items() if buf == "W" and off >= lo)
    ends = [o for o, _, _ in ents[1:]] + [net.nW]
    return [(n, o, e, a) for (o, n, a), e in zip(ents, ends)]


def trainer_oracle(torch, tr, name, net, W0, Wg, variables):
    """The first step from zero slots on float64 device tensors, slicing by param_index: ({name: ratio}, W)."""
    wd = tr.wd_l2
    w, g = W0.double(), Wg.double()
    gp = OC.opt_grad(w, g, wd)
    if name == "sgd":
        x = gp
    else:
        _, m, v = OC.adam_step(w, g, 0.0, 0.0, 1, tr.lr, tr.adam_beta1, tr.adam_beta2, tr.adam_eps, wd, tr.wd_decoupled)
        b1, b2 = OC.f32(tr.adam_beta1), OC.f32(tr.adam_beta2)
        x = (m / (1.0 - b1)) / ((v / (1.0 - b2)) ** 0.5 + OC.f32(tr.adam_eps)) + OC.f32(tr.wd_decoupled) * w
    sw = torch.stack([(w[o:e] ** 2).sum() for _, o, e, _ in variables]).sqrt()
    sx = torch.stack([(x[o:e] ** 2).sum() for _, o, e, _ in variables]).sqrt()
    ad = torch.tensor([a for _, _, _, a in variables], device=w.device)
    r = torch.where(ad & (sw > 0) & (sx > 0), OC.f32(tr.trust_coeff) * sw / sx, torch.ones_like(sw))
    lens = torch.tensor([e - o for _, o, e, _ in variables], device=w.device)
    lo = variables[0][1]
    re_ = torch.ones_like(w)
    re_[lo:] = torch.repeat_interleave(r, lens)
    if name == "sgd":
        w1, _ = OC.sgd_step(w, re_ * gp, 0.0, tr.lr, momentum=tr.sgd_momentum, nesterov=tr.sgd_nesterov)
    else:
        w1 = w - OC.f32(tr.lr) * (re_ * x)
    return dict(zip([n for n, _, _, _ in variables], r.tolist())), w1


@pytest.mark.parametrize("name", sorted(TRAINER))
def test_trainer_step_against_the_oracle(gpu, name):
    torch, l = gpu
    net, tr = GC.make_trainer(torch, False, **TRAINER[name])
    assert tr.opt_ranges == [("W", 0, net.nW, 1), ("Bt", 0, net.nBt, 1)] and sorted(tr._trust_plans) == [0]
    variables = w_variables(net)
    W0 = net.W.clone()
    tr.run_eager_once()
    torch.cuda.synchronize()
    grads = net.G.clone()
    tr._optimizer()
    torch.cuda.synchronize()
    assert int(tr.match_status().max()) == 0 and int(tr.skipped_steps) == 0
    got = tr.trust_ratios()
    want, W1 = trainer_oracle(torch, tr, name, net, W0, net.Wg, variables)
    assert list(got) == [n for n, _, _, _ in variables] and len(got) == sum(1 for b, *_ in net.param_index.values() if b == "W")
    biases = [n for n, _, _, a in variables if not a]
    assert biases and all(n.endswith("/biases") for n in biases) and all(got[n] == 1.0 for n in biases)
    rel = max(abs(got[n] / want[n] - 1) for n in got)
    err = ((net.W.double() - W1).abs() / (ATOL + RTOL * W1.abs())).max().item()
    moved = (W1 - W0.double()).abs().max().item()
    lo, med, hi = tr.trust_ratio_stats()
    print("%s: %d variables, ratios %.3g / %.3g / %.3g, worst ratio error %.3g, W worst error %.3g x bar, largest update %.3g" % (
        name, len(got), lo, med, hi, rel, err, moved))
    assert rel <= RATIO_RTOL and err <= 1.0 and moved > 10 * ATOL
    assert sum(1 for n in got if got[n] != 1.0) == len(got) - len(biases) and lo <= med <= hi
    # the betas: the same trainer without the key, on the same gradients
    bt = [t.clone() for t in (net.Bt, tr.Btmom, tr.Btema) + ((tr.Btms,) if tr.Btms is not None else ())]
    w_trusted = net.W.clone()
    del tr, net
    torch.cuda.empty_cache()
    net2, tr2 = GC.make_trainer(torch, False, **without_trust(TRAINER[name]))
    assert GC.same_bits(torch, net2.W, W0) and tr2.trust_ratios() is None and tr2.trust_ratio_stats() is None
    net2.zero_grads()
    net2.G.copy_(grads)
    tr2._optimizer()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(bt, (net2.Bt, tr2.Btmom, tr2.Btema) + ((tr2.Btms,) if tr2.Btms is not None else ()))):
        assert GC.same_bits(torch, a, b), i
    assert not torch.equal(net2.W, w_trusted) and not torch.equal(net2.Bt, torch.zeros_like(net2.Bt))


def test_trainable_scopes_select_the_variables(gpu):
    torch, l = gpu
    from multibox_amd.engine import Net
    probe = w_variables(Net(batch=2, input_size=299, k=5, mode="train", seed=5))
    scope = probe[len(probe) // 2][0].rsplit("/", 2)[0]       # the block around a variable in the middle of the network
    inside = [(n, o, e, a) for n, o, e, a in probe if re.match(scope, n)]
    assert 0 < len(inside) < len(probe), scope
    del probe
    net, tr = GC.make_trainer(torch, False, trainable_scopes=[scope], **TRAINER["sgd"])
    W0 = net.W.clone()
    tr.run_eager_once()
    tr._optimizer()
    torch.cuda.synchronize()
    got = tr.trust_ratios()
    assert sorted(got) == sorted(n for n, _, _, _ in inside), scope
    assert all((got[n] != 1.0) == a for n, _, _, a in inside)
    mask = torch.zeros(net.nW, dtype=torch.bool, device="cuda")
    for n, o, e, a in inside:
        mask[o:e] = True
    changed = net.W.view(torch.int32) != W0.view(torch.int32)
    assert not bool((changed & ~mask).any()) and int(changed.sum()) > 1000
    print("scope %s: %d of %d variables, %d elements changed" % (scope, len(inside), len(w_variables(net)), int(changed.sum())))


def test_trainer_without_the_key_launches_nothing_new(gpu):
    torch, l = gpu
    from multibox_amd import _lib
    rec = GC.Recorder(l)
    _lib._lib = rec
    try:
        net, tr = GC.make_trainer(torch, False, **without_trust(TRAINER["sgd"]))
        tr.run_eager_once()
        tr._optimizer()
        torch.cuda.synchronize()
        off = list(rec.names)
        rec.names.clear()
        del net, tr
        torch.cuda.empty_cache()
        net2, tr2 = GC.make_trainer(torch, False, **TRAINER["sgd"])
        tr2.run_eager_once()
        tr2._optimizer()
        torch.cuda.synchronize()
        on = list(rec.names)
    finally:
        _lib._lib = l
    assert not TRUST_ENTRIES & set(off) and off.count("mbx_sgd_ema_step") == 2
    # with the key: the filters' launch exchanged for the three passes, the betas' stays
    assert [on.count(x) for x in ("mbx_trust_norms_sgd", "mbx_trust_ratios", "mbx_sgd_ema_step_trust")] == [1, 1, 1]
    assert on.count("mbx_sgd_ema_step") == 1 and on.count("mbx_trust_plan") == 1
    strip = lambda names: [x for x in names if x not in TRUST_ENTRIES and x != "mbx_sgd_ema_step"]
    assert strip(on) == strip(off)


@pytest.mark.parametrize("name", sorted(TRAINER))
def test_checkpoint_resumes_to_the_same_bytes(gpu, tmp_path, name):
    """No format change: the rule name and the slots mean what they meant.  Save after one step, restore into a fresh Trainer,
    apply the second step's optimiser phase to the gradients the first Trainer computed for it: the uninterrupted run's bytes."""
    torch, l = gpu
    from multibox_amd import checkpoint as CK
    kw = TRAINER[name]
    net, tr = GC.make_trainer(torch, False, **kw)
    tr.step()
    torch.cuda.synchronize()
    path = CK.save(str(tmp_path), tr)
    st = torch.load(path, map_location="cpu")
    assert st["optimizer"] == name and st["global_step"] == 1 and st["opt_steps"] == 1
    assert not [k for k in st if "trust" in k.lower()]
    del st
    tr.run_eager_once()
    torch.cuda.synchronize()
    grads = net.G.clone()
    tr._optimizer()
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in GO.state_of(net, tr).items() if k in GO.CKPT_COMPARED}
    ratios = tr.trust_ratios()
    del tr, net
    torch.cuda.empty_cache()
    net2, tr2 = GC.make_trainer(torch, False, **kw)
    CK.restore_for_training(path, tr2)
    assert tr2.global_step == 1 and tr2.optimizer_steps() == 1 and not tr2.events
    net2.zero_grads()
    net2.G.copy_(grads)
    tr2._optimizer()
    torch.cuda.synchronize()
    got = GO.state_of(net2, tr2)
    for k, v in want.items():
        assert GC.same_bits(torch, got[k], v), k
    assert tr2.trust_ratios() == ratios


# ------------------------------------------------------------------------------------------------------ data parallel
def _dp_worker(port, out_dir):
    """One rank with a real process group and MBX_FORCE_DIST=1: the bucketed all-reduce sits between the backward pass and the
    optimiser phase, and the trust passes run behind it on the reduced buffers."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", MBX_FORCE_DIST="1")
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=0, world_size=1)
    torch.cuda.set_device(0)
    net, tr = GC.make_trainer(torch, False, process_group=dist.group.WORLD, **TRAINER["sgd"])
    assert tr.reducer.enabled and len(tr._segments) > 1
    tr.step()
    torch.cuda.synchronize()
    torch.save({"G": net.G.cpu(), "W": net.W.cpu(), "Bt": net.Bt.cpu(), "Wmom": tr.Wmom.cpu(), "ratios": tr.trust_ratios(),
                "status": int(tr.match_status().max()), "skipped": int(tr.skipped_steps)}, os.path.join(out_dir, "rank0.pt"))
    dist.destroy_process_group()


def test_data_parallel_world_of_one_gives_the_single_process_bytes(gpu, tmp_path):
    """The step of a rank behind the (forced) all-reduce against the optimiser phase of a trainer without a process group on the
    rank's reduced gradients: ratios, filters, accumulator and betas to the bit."""
    torch, l = gpu
    import os
    import torch.multiprocessing as mp
    p = mp.get_context("spawn").Process(target=_dp_worker, args=(29800 + os.getpid() % 1000, str(tmp_path)))
    p.start()
    p.join(300)
    assert p.exitcode == 0
    r = torch.load(tmp_path / "rank0.pt")
    assert r["status"] == 0 and r["skipped"] == 0
    net, tr = GC.make_trainer(torch, False, **TRAINER["sgd"])
    w0 = net.W.clone()
    net.zero_grads()
    net.G.copy_(r["G"].cuda())
    tr._optimizer()
    torch.cuda.synchronize()
    assert tr.trust_ratios() == r["ratios"] and len(r["ratios"]) == len(w_variables(net))
    for name, mine in (("W", net.W), ("Bt", net.Bt), ("Wmom", tr.Wmom)):
        assert GC.same_bits(torch, mine.cpu(), r[name]), name
    assert not torch.equal(net.W, w0)
