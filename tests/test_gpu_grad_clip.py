"""GPU: global-norm gradient clipping and the non-finite-step guard (mbx_grad_sqnorm, mbx_clip_finalize,
mbx_rmsprop_ema_step_clipped, Trainer(clip_gradient_norm=...)) against tests/clip_oracle.py.

Bars.  Norm: rtol 1e-6 against the float64 oracle -- the value is one float32 rounding of each g' (2^-24 relative), double
accumulation and one float32 rounding of the result, about 1.2e-7 in all.  Clipped update: the existing optimiser test's
rtol 1e-5 / atol 1e-6 against oracle.ref_numpy.rmsprop_step.  Everything else is exact: a scale of 1 has the bits of 1.0f
and gives the bytes of mbx_rmsprop_ema_step, two runs give the same bytes, a skipped step changes no byte.

Sizes: the smallest at which each path of the kernels can go wrong -- 1; 3 (tail only); 4 * 64 + 3 aligned and with every
pointer moved by one float (the element-by-element path); 100003 (many workgroups and a tail); one and two grid strides of
16-byte groups plus 4 * 64 + 3 (the norm kernel takes two strides per iteration), computed from mbx_grad_sqnorm_partials.
"""
import numpy as np
import pytest

from tests import clip_oracle as CO

pytestmark = pytest.mark.gpu

ONE_BITS = np.float32(1.0).tobytes()
WD = 4e-5


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from multibox_amd import _lib
    return torch, _lib.lib()


def S():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sizes(l):
    """(n, offset in floats) of the module docstring."""
    stride = 4 * 256 * int(l.mbx_grad_sqnorm_partials(1 << 40))          # elements one grid stride of 16-byte groups covers
    assert int(l.mbx_grad_sqnorm_partials(stride)) == stride // 1024      # ... and the grid is at its cap there
    return [(1, 0), (3, 0), (259, 0), (259, 1), (100003, 0), (stride + 259, 0), (2 * stride + 259, 0)]


N_SIZES = 7


def dev(torch, a, off=0):
    """A float32 device copy of `a` whose first element sits `off` floats behind a 16-byte boundary."""
    t = torch.zeros(len(a) + off, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[off:]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return v


def same_bits(torch, a, b):
    """Byte equality of two device tensors (NaNs and signed zeros included)."""
    as_int = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else t.dtype)
    return a.dtype == b.dtype and torch.equal(as_int(a), as_int(b))


def norm_block(gpu, ranges, max_norm, ctl=(0.0, 0.0), counts=None):
    """mbx_grad_sqnorm per range into consecutive slots, one mbx_clip_finalize.  ranges: [(g, w | None, wd)] device tensors.
    Returns (clip block [8] float32, partials float64, counts int64[2]) as numpy plus the device clip block."""
    torch, l = gpu
    from multibox_amd import _lib
    slots = [int(l.mbx_grad_sqnorm_partials(g.numel())) for g, _, _ in ranges]
    part = torch.full((sum(slots),), -1.0, dtype=torch.float64, device="cuda")
    clip = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda") if counts is None else counts
    c = torch.tensor(ctl, dtype=torch.float32, device="cuda")
    at = 0
    for (g, w, wd), k in zip(ranges, slots):
        _lib.check(l.mbx_grad_sqnorm(g.data_ptr(), None if w is None else w.data_ptr(), g.numel(), wd,
                                     part.data_ptr() + 8 * at, S()), "grad_sqnorm")
        at += k
    _lib.check(l.mbx_clip_finalize(part.data_ptr(), at, max_norm, c.data_ptr(), clip.data_ptr(), cnt.data_ptr(), S()), "clip_finalize")
    assert c.tolist() == list(ctl)                            # the control block is only read
    return clip.cpu().numpy(), part.cpu().numpy(), cnt.cpu().numpy(), clip


def data(n, seed, w_scale=1e5):
    rng = np.random.RandomState(seed)
    return (rng.randn(n) * 10).astype(np.float32), (rng.randn(n) * w_scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("case", range(N_SIZES))
@pytest.mark.parametrize("wd", [0.0, WD])
def test_norm_against_the_oracle_and_reproducible(gpu, case, wd):
    torch, l = gpu
    n, off = sizes(l)[case]
    g, w = data(n, case)                                      # |wd * w| ~ 4: a norm that forgot the decay term is far off
    dg, dw = dev(torch, g, off), (dev(torch, w, off) if wd else None)
    want = CO.global_norm([(g, w, wd)])
    runs = [norm_block(gpu, [(dg, dw, wd)], want * 2)[:3] for _ in range(2)]
    clip, part, cnt = runs[0]
    print("n=%d off=%d wd=%g: norm %r oracle %r rel %.3g" % (n, off, wd, float(clip[3]), want, abs(float(clip[3]) - want) / want))
    assert np.isclose(float(clip[3]), want, rtol=1e-6, atol=0)
    assert np.isclose(float(np.sqrt(part.sum())), want, rtol=1e-6, atol=0) and (part >= 0).all()
    assert clip[:3].tobytes() == np.array([0, 0, 1], np.float32).tobytes() and clip[4] == 0 and not clip[5:].any()
    assert cnt.tolist() == [0, 0]
    assert runs[1][0].tobytes() == clip.tobytes() and runs[1][1].tobytes() == part.tobytes()
    if wd:
        assert not np.isclose(float(clip[3]), CO.global_norm([(g, None, 0.0)]), rtol=1e-3)


def test_two_ranges_feed_one_finalize(gpu):
    torch, l = gpu
    (ga, wa), (gb, _) = data(100003, 11), data(259, 12)
    ranges = [(dev(torch, ga), dev(torch, wa), WD), (dev(torch, gb, 1), None, 0.0)]
    want, scale, _ = CO.clip([(ga, wa, WD), (gb, None, 0.0)], 3.0)
    runs = [norm_block(gpu, ranges, 3.0)[:3] for _ in range(2)]
    clip, part, cnt = runs[0]
    print("two ranges: norm %r oracle %r scale %r oracle %r" % (clip[3], want, clip[2], scale))
    assert len(part) == int(l.mbx_grad_sqnorm_partials(100003)) + 1
    assert np.isclose(float(clip[3]), want, rtol=1e-6, atol=0) and np.isclose(float(clip[2]), scale, rtol=1e-6, atol=0)
    assert clip[4] == 1 and cnt.tolist() == [1, 0]
    assert np.allclose(clip, CO.clip_block([(ga, wa, WD), (gb, None, 0.0)], 3.0), rtol=1e-6, atol=0)
    assert runs[1][0].tobytes() == clip.tobytes() and runs[1][1].tobytes() == part.tobytes()


# ------------------------------------------------------------------------------------------------------ the optimiser
HYPER = dict(lr=0.0094, decay=0.9, eps=1.0, d=0.999)


class State:
    """w, g, ms, mom, ema, wb, reg of one flat range on the device, every pointer `off` floats behind a 16-byte boundary."""

    def __init__(self, torch, w, g, off=0):
        n = len(w)
        self.n, self.w, self.g = n, dev(torch, w, off), dev(torch, g, off)
        self.ms, self.mom, self.ema = dev(torch, np.ones(n), off), dev(torch, np.full(n, 0.25), off), dev(torch, w * 0.5, off)
        self.wb = torch.zeros(n + 2 * off, dtype=torch.bfloat16, device="cuda")[2 * off:]
        self.reg = torch.zeros(1, dtype=torch.float32, device="cuda")

    def tensors(self):
        return (self.w, self.ms, self.mom, self.ema, self.wb, self.reg)

    def snapshot(self):
        return [t.clone() for t in self.tensors()]

    def step(self, l, momentum, wd, clip=None, ctl=None, trainable=1):
        from multibox_amd import _lib
        a = [self.w.data_ptr(), self.g.data_ptr(), self.ms.data_ptr(), self.mom.data_ptr() if momentum else None,
             self.ema.data_ptr(), self.wb.data_ptr(), self.n, HYPER["lr"], HYPER["decay"], momentum, HYPER["eps"], wd, HYPER["d"],
             trainable, self.reg.data_ptr()]
        if clip is None:
            _lib.check(l.mbx_rmsprop_ema_step(*a, None if ctl is None else ctl.data_ptr(), S()), "rmsprop")
        else:
            _lib.check(l.mbx_rmsprop_ema_step_clipped(*a, clip.data_ptr(), S()), "rmsprop clipped")


@pytest.mark.parametrize("case", range(N_SIZES))
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_scale_one_is_byte_identical_to_the_plain_step(gpu, case, momentum):
    """reg_loss is summed over workgroups with float atomics, whose order is free: the weights here are small integers and the
    decay a power of two, so every partial sum of w^2 is exact (< 2^24) and its bytes do not depend on that order.  The
    gradients are arbitrary reals, and after the first of the two steps so are the weights of everything but reg_loss."""
    torch, l = gpu
    n, off = sizes(l)[case]
    rng = np.random.RandomState(100 + case)
    w, g = rng.randint(-2, 3, n).astype(np.float32), (rng.randn(n) * 10).astype(np.float32)
    wd = 2.0 ** -14
    plain, clipped = State(torch, w, g, off), State(torch, w, g, off)
    clip, _, cnt, dclip = norm_block(gpu, [(clipped.g, clipped.w, wd)], float("inf"))
    assert clip[2:3].tobytes() == ONE_BITS and clip[4] == 0 and cnt.tolist() == [0, 0]
    plain.step(l, momentum, wd)
    clipped.step(l, momentum, wd, clip=dclip)
    for name, a, b in zip(("w", "ms", "mom", "ema", "wb", "reg_loss"), plain.tensors(), clipped.tensors()):
        assert same_bits(torch, a, b), name
    assert not torch.equal(plain.w, dev(torch, w, off))
    assert float(plain.reg) == 0.5 * wd * float((w.astype(np.float64) ** 2).sum())         # exact, as said above
    # a second step on real-valued weights (reg_loss left out: see above)
    plain.step(l, momentum, wd)
    clipped.step(l, momentum, wd, clip=dclip)
    for name, a, b in zip(("w", "ms", "mom", "ema", "wb"), plain.tensors(), clipped.tensors()):
        assert same_bits(torch, a, b), name


@pytest.mark.parametrize("case", range(N_SIZES))
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_clipped_step_against_the_numpy_optimiser(gpu, case, momentum):
    torch, l = gpu
    from oracle import ref_numpy as R
    n, off = sizes(l)[case]
    g, w = data(n, 200 + case, w_scale=1.0)
    w = (w * 1e4).astype(np.float32)                          # wd * w ~ 0.4 beside g ~ 10
    st = State(torch, w, g, off)
    norm, scale, _ = CO.clip([(g, w, WD)], 0.5 * CO.global_norm([(g, w, WD)]))
    clip, _, cnt, dclip = norm_block(gpu, [(st.g, st.w, WD)], 0.5 * norm)
    assert np.isclose(float(clip[2]), 0.5, rtol=1e-6) and clip[4] == 1 and cnt.tolist() == [1, 0]
    st.step(l, momentum, WD, clip=dclip)
    ms, mom, ema = np.ones(n, np.float32), np.full(n, 0.25, np.float32), (w * 0.5).astype(np.float32)
    if not momentum:
        mom = np.zeros(n, np.float32)
    reg_ref = 0.5 * WD * float((w.astype(np.float64) ** 2).sum())
    ema -= np.float32(1 - HYPER["d"]) * (ema - w)
    gi = (np.float32(clip[2]) * (g + np.float32(WD) * w)).astype(np.float32)
    wr = w.copy()
    R.rmsprop_step(wr, gi, ms, mom, HYPER["lr"], HYPER["decay"], momentum, HYPER["eps"])
    err = np.abs(st.w.cpu().numpy() - wr) / (1e-6 + 1e-5 * np.abs(wr))
    print("n=%d off=%d momentum=%g: scale %r, worst weight error %.3g x bar" % (n, off, momentum, clip[2], err.max()))
    assert np.allclose(st.w.cpu().numpy(), wr, rtol=1e-5, atol=1e-6)
    assert np.allclose(st.ms.cpu().numpy(), ms, rtol=1e-5)
    assert np.allclose(st.ema.cpu().numpy(), ema, rtol=1e-5, atol=1e-6)
    if momentum:
        assert np.allclose(st.mom.cpu().numpy(), mom, rtol=1e-5, atol=1e-6)
    assert np.isclose(float(st.reg), reg_ref, rtol=1e-4)
    assert torch.equal(st.wb.float(), st.w.to(torch.bfloat16).float())
    # the unclipped update differs: the scale was used
    assert not np.allclose(st.ms.cpu().numpy(), np.float32(0.9) + np.float32(0.1) * (g + np.float32(WD) * w) ** 2, rtol=1e-3)
    # a frozen range: no update (EMA, regulariser and bf16 refresh only)
    w0, ms0 = st.w.clone(), st.ms.clone()
    st.step(l, momentum, WD, clip=dclip, trainable=0)
    assert torch.equal(st.w, w0) and torch.equal(st.ms, ms0)


# ------------------------------------------------------------------------------------------------------ magnitude, exactness
def test_huge_and_tiny_gradients(gpu):
    torch, l = gpu
    n = 1000
    g = np.full(n, 3e19, np.float32)                          # a float32 square would overflow
    st = State(torch, np.zeros(n, np.float32), g)
    want = CO.global_norm([(g, None, 0.0)])
    clip, _, cnt, dclip = norm_block(gpu, [(st.g, None, 0.0)], 1.0)
    print("3e19: norm %r oracle %r scale %r oracle %r" % (clip[3], want, clip[2], 1.0 / want))
    assert np.isfinite(clip[3]) and np.isclose(float(clip[3]), want, rtol=1e-6, atol=0)
    assert np.isclose(float(clip[2]), 1.0 / want, rtol=1e-6, atol=0) and clip[2] > 0
    assert clip[1] == 0 and clip[4] == 1 and cnt.tolist() == [1, 0]
    st.step(l, 0.0, 0.0, clip=dclip)
    for t in (st.w, st.ms, st.ema):
        assert bool(torch.isfinite(t).all())
    # the clipped vector has norm max_norm = 1: every element 1 / sqrt(n)
    gi = np.float32(clip[2]) * g
    assert np.allclose(st.ms.cpu().numpy(), np.float32(0.9) + np.float32(0.1) * gi * gi, rtol=1e-5)
    assert np.isclose(float(np.sqrt((gi.astype(np.float64) ** 2).sum())), 1.0, rtol=1e-5)
    g = np.full(n, 1e-30, np.float32)                         # its square is far below the smallest float32
    want = CO.global_norm([(g, None, 0.0)])
    clip, _, cnt, _ = norm_block(gpu, [(dev(torch, g), None, 0.0)], 1.0)
    print("1e-30: norm %r oracle %r" % (clip[3], want))
    assert clip[3] > 0 and np.isclose(float(clip[3]), want, rtol=1e-6, atol=0)
    assert clip[2:3].tobytes() == ONE_BITS and clip[4] == 0 and cnt.tolist() == [0, 0]
    clip, _, cnt, _ = norm_block(gpu, [(dev(torch, np.zeros(n)), None, 0.0)], 1.0)      # a norm of 0: scale 1
    assert clip[3] == 0 and clip[2:3].tobytes() == ONE_BITS and clip[4] == 0 and clip[1] == 0 and cnt.tolist() == [0, 0]


def test_scale_is_exactly_one_below_the_bound(gpu):
    torch, l = gpu
    g, w = data(259, 3)
    norm = CO.global_norm([(g, w, WD)])
    cnt = torch.tensor([5, 9], dtype=torch.int64, device="cuda")
    for max_norm in (norm * (1 + 1e-6), norm * 2, 1e30, float("inf")):
        clip = norm_block(gpu, [(dev(torch, g), dev(torch, w), WD)], max_norm, counts=cnt)[0]
        assert clip[2:3].tobytes() == ONE_BITS and clip[4] == 0 and clip[0] == 0 and clip[1] == 0, max_norm
        assert cnt.tolist() == [5, 9]
    big = np.full(259, 3e19, np.float32)
    clip = norm_block(gpu, [(dev(torch, big), None, 0.0)], float("inf"), counts=cnt)[0]        # inf never clips
    assert clip[2:3].tobytes() == ONE_BITS and clip[4] == 0 and np.isfinite(clip[3]) and cnt.tolist() == [5, 9]
    clip = norm_block(gpu, [(dev(torch, g), dev(torch, w), WD)], norm * (1 - 1e-5), counts=cnt)[0]
    assert clip[2] < 1 and clip[4] == 1 and cnt.tolist() == [6, 9]


# ------------------------------------------------------------------------------------------------------ non-finite, flagged
def gated_launches_change_nothing(gpu, st, dclip):
    torch, l = gpu
    from multibox_amd import _lib
    before = st.snapshot()
    st.step(l, 0.9, WD, clip=dclip)
    _lib.check(l.mbx_ema_update(st.ema.data_ptr(), st.w.data_ptr(), st.n, HYPER["d"], dclip.data_ptr(), S()), "ema_update")
    torch.cuda.synchronize()
    for name, a, b in zip(("w", "ms", "mom", "ema", "wb", "reg_loss"), before, st.tensors()):
        assert same_bits(torch, a, b), name


@pytest.mark.parametrize("where,value", [("tail", float("nan")), ("vector", float("inf")), ("vector", -float("inf")),
                                         ("tail", float("inf"))])
@pytest.mark.parametrize("ctl1", [0.0, 2.0])
def test_non_finite_gradient_skips_the_step(gpu, where, value, ctl1):
    torch, l = gpu
    n = 259                                                   # 64 16-byte groups and a tail of 3
    g, w = data(n, 7, w_scale=1e3)
    g[n - 1 if where == "tail" else 5] = value
    st = State(torch, w, g)
    cnt = torch.tensor([4, 6], dtype=torch.int64, device="cuda")
    clip, _, _, dclip = norm_block(gpu, [(st.g, st.w, WD)], 1.0, ctl=(0.0, ctl1), counts=cnt)
    assert clip[0] == 0 and clip[1] == ctl1 + 1 and clip[4] == 0
    # an already flagged step has its cause: no count; otherwise this one is the guard's
    assert cnt.tolist() == ([4, 7] if ctl1 == 0 else [4, 6])
    gated_launches_change_nothing(gpu, st, dclip)


@pytest.mark.parametrize("ctl", [(1.0, 0.0), (0.0, 2.0)])
def test_flagged_control_block_is_copied_through(gpu, ctl):
    torch, l = gpu
    g, w = data(259, 8, w_scale=1e3)
    st = State(torch, w, g)
    cnt = torch.tensor([4, 6], dtype=torch.int64, device="cuda")
    clip, _, _, dclip = norm_block(gpu, [(st.g, st.w, WD)], 1.0, ctl=ctl, counts=cnt)       # would clip: the norm is ~160
    assert clip[:2].tolist() == list(ctl) and clip[4] == 1 and clip[2] < 1
    assert cnt.tolist() == [4, 6]
    gated_launches_change_nothing(gpu, st, dclip)
    # the same block with a clear control block applies the step
    clip, _, _, dclip = norm_block(gpu, [(st.g, st.w, WD)], 1.0, counts=cnt)
    w0 = st.w.clone()
    st.step(l, 0.9, WD, clip=dclip)
    assert cnt.tolist() == [5, 6] and not torch.equal(st.w, w0)


# ------------------------------------------------------------------------------------------------------ through the Trainer
def trainer_batch(torch):
    """The batch of test_trainer_step_focal_graph_equals_eager."""
    from multibox_amd import priors as PR
    priors = np.array(PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.]), np.float32)
    gen = torch.Generator().manual_seed(3)
    images = torch.rand(2, 299, 299, 3, generator=gen) * 2 - 1
    rng = np.random.RandomState(1)
    n_gt = np.array([3, 0], np.int32)
    gt = np.zeros((2, 13, 4), np.float32)
    xy = rng.uniform(0, .7, (3, 2)); wh = rng.uniform(.05, .3, (3, 2))
    gt[0, :3, :2] = xy; gt[0, :3, 2:] = xy + wh
    return priors, images, gt, n_gt


def make_trainer(torch, use_graph, **kw):
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer
    priors, images, gt, n_gt = trainer_batch(torch)
    net = Net(batch=2, input_size=299, k=5, mode="train", seed=5)
    tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, **kw)
    tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
    return net, tr


def params(net):
    return net.W.cpu().numpy().copy(), net.Bt.cpu().numpy().copy()


@pytest.mark.parametrize("use_graph", [True, False])
def test_trainer_clips_and_guards(gpu, use_graph):
    torch, l = gpu
    from multibox_amd.engine import WEIGHT_DECAY
    from oracle import ref_numpy as R
    # 1. inf: the norm is reported, nothing is clipped
    net, tr = make_trainer(torch, use_graph, clip_gradient_norm=float("inf"))
    assert tr.opt_ranges == [("W", 0, net.nW, 1), ("Bt", 0, net.nBt, 1)]
    W0, Bt0 = params(net)
    tr.step()
    torch.cuda.synchronize()
    assert int(tr.match_status().max()) == 0
    Wg, Btg = net.Wg.cpu().numpy(), net.Btg.cpu().numpy()[:net.nBt]
    ranges = [(Wg, W0, WEIGHT_DECAY), (Btg, None, 0.0)]
    norm = CO.global_norm(ranges)
    print("graph=%d: grad_norm %r oracle %r" % (use_graph, tr.grad_norm(), norm))
    assert np.isfinite(norm) and norm > 0 and np.isclose(tr.grad_norm(), norm, rtol=1e-6, atol=0)
    assert tr.clip_scale() == 1.0 and tr.clipped_steps() == 0 and tr.nonfinite_steps() == 0
    assert int(tr.skipped_steps) == 0 and tr.fold_skipped() == 0
    W1 = net.W.cpu().numpy()
    assert not np.array_equal(W1, W0)
    del tr, net
    # 2. half of that norm: clipped, and the update is the oracle's with that scale
    net, tr = make_trainer(torch, use_graph, clip_gradient_norm=0.5 * norm)
    W0b, Bt0b = params(net)
    assert W0b.tobytes() == W0.tobytes() and Bt0b.tobytes() == Bt0.tobytes()           # same seed
    tr.step()
    torch.cuda.synchronize()
    scale, own = tr.clip_scale(), tr.grad_norm()
    print("graph=%d: clip_scale %r = %r / %r" % (use_graph, scale, 0.5 * norm, own))
    assert scale < 1 and np.isclose(scale, 0.5 * norm / own, rtol=1e-6, atol=0)
    assert np.isclose(own, norm, rtol=1e-3)                   # (another run of the same step: its atomics may add in another order)
    assert tr.clipped_steps() == 1 and tr.nonfinite_steps() == 0 and int(tr.skipped_steps) == 0
    Wg, Btg = net.Wg.cpu().numpy(), net.Btg.cpu().numpy()[:net.nBt]
    for name, now, p0, g, wd in (("W", net.W, W0, Wg, WEIGHT_DECAY), ("Bt", net.Bt, Bt0, Btg, 0.0)):
        gi = (np.float32(scale) * (g + np.float32(wd) * p0)).astype(np.float32)
        ref = p0.copy()
        R.rmsprop_step(ref, gi, np.ones_like(ref), np.zeros_like(ref), tr.lr, tr.rms_decay, 0.0, tr.eps)
        got = now.cpu().numpy()
        err = np.abs(got - ref) / (1e-6 + 1e-5 * np.abs(ref))
        print("graph=%d %s: worst error %.3g x bar, largest update %.3g" % (use_graph, name, err.max(), np.abs(ref - p0).max()))
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-6), name
        assert np.abs(ref - p0).max() > 1e-5, name
    assert not np.array_equal(net.W.cpu().numpy(), W1)        # not the unclipped update
    # 3. an Inf in one filter gradient after the backward pass: the optimiser phase changes nothing and counts the skip
    net.Wg[12345] = float("inf")
    state = lambda: [t.clone() for t in (net.W, net.Bt, net.Wb, tr.Wms, tr.Btms, tr.Wema, tr.Btema, net.MM, net.MV, tr.MMema, tr.MVema)]
    before = state()
    tr._optimizer()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(before, state())):
        assert same_bits(torch, a, b), i
    assert int(tr.skipped_steps) == 1 and tr.nonfinite_steps() == 1 and tr.clipped_steps() == 1
    assert net.step_ctl[:2].tolist() == [0.0, 0.0]            # the real control block is never written
    tr.global_step += 1                                       # (what step() does behind _optimizer)
    assert tr.fold_skipped() == 1 and tr.global_step == 1
    assert tr.events[-1]["event"] == "skipped_steps" and tr.events[-1]["nonfinite_steps"] == 1


class Recorder:
    """Stands in for the loaded library: hands every attribute on and notes the entry points asked for."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


NEW = {"mbx_grad_sqnorm", "mbx_grad_sqnorm_partials", "mbx_clip_finalize", "mbx_rmsprop_ema_step_clipped"}


def test_trainer_without_the_key_launches_nothing_new(gpu):
    torch, l = gpu
    from multibox_amd import _lib
    rec = Recorder(l)
    _lib._lib = rec
    try:
        net, tr = make_trainer(torch, False)
        tr.step()
        torch.cuda.synchronize()
        off = list(rec.names)
        rec.names.clear()
        net2, tr2 = make_trainer(torch, False, clip_gradient_norm=float("inf"))
        tr2.step()
        torch.cuda.synchronize()
        on = list(rec.names)
    finally:
        _lib._lib = l
    assert tr.grad_norm() is None and tr.clip_scale() is None and tr.clipped_steps() is None and tr.nonfinite_steps() is None
    assert not NEW & set(off) and off.count("mbx_rmsprop_ema_step") == 2 and "mbx_bn_moving_update" in off
    # with the key: the same sequence with the optimiser phase's launches exchanged
    assert on.count("mbx_grad_sqnorm") == 2 and on.count("mbx_clip_finalize") == 1 and on.count("mbx_rmsprop_ema_step_clipped") == 2
    assert "mbx_rmsprop_ema_step" not in on
    strip = lambda names: [x for x in names if x not in NEW and x != "mbx_rmsprop_ema_step"]
    assert strip(on) == strip(off)
    assert tr2.clip_scale() == 1.0 and net2 is not net
