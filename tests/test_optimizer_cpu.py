"""OPTIMIZER / LEARNING_RATE_WARMUP_STEPS without a device: the config keys, the warm-up factor, the ctypes signatures and the
argument checks of mbx_sgd_ema_step / mbx_adam_ema_step (they come before any launch), and the oracles of the two rules.

The oracles (sgd_step, adam_step, ema_step) are plain arithmetic on whatever arrays they are handed: float64 numpy arrays are
the anchor tests/test_gpu_optimizer.py compares the kernels with, float32 ones the restatement checked here, and float64
torch tensors serve the trainer-level tests (60 M elements).  Hyper-parameters enter as the float32 values the C ABI hands the
kernel; the bias corrections are computed in double, as the kernel does.
"""
import ctypes as C

import numpy as np
import pytest

INVALID = -1                                                   # MBX_ERR_INVALID_ARG (include/mbx.h)
RTOL, ATOL = 1e-5, 1e-6                                        # the optimiser bar of tests/test_gpu_grad_clip.py


# ------------------------------------------------------------------------------------------------------ oracles
def f32(x):
    """The value a float hyper-parameter has once it went through the C ABI."""
    return float(np.float32(x))


def opt_grad(w, g, wd=0.0, scale=None):
    """g' = g + wd * w, times the clip scale (the float32 word clip[2]) when given."""
    gp = g + f32(wd) * w if wd else g
    return gp if scale is None else f32(scale) * gp


def sgd_step(w, g, acc, lr, momentum=0.9, nesterov=False, wd=0.0, scale=None):
    """tf.train.MomentumOptimizer: acc = momentum * acc + g'; w -= lr * acc, or lr * (g' + momentum * acc) with nesterov.
    momentum 0: w -= lr * g', no accumulator (acc is passed through).  Returns (w, acc)."""
    gp = opt_grad(w, g, wd, scale)
    if not momentum:
        return w - f32(lr) * gp, acc
    acc = f32(momentum) * acc + gp
    return w - f32(lr) * ((gp + f32(momentum) * acc) if nesterov else acc), acc


def adam_step(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, wd_decoupled=0.0, scale=None):
    """Adam's step number t (1 = the first applied step); wd_decoupled != 0: AdamW.  Returns (w, m, v)."""
    b1, b2 = f32(beta1), f32(beta2)
    gp = opt_grad(w, g, wd, scale)
    m = b1 * m + (1.0 - b1) * gp
    v = b2 * v + (1.0 - b2) * gp * gp
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    upd = (m / bc1) / ((v / bc2) ** 0.5 + f32(eps))
    if wd_decoupled:
        upd = upd + f32(wd_decoupled) * w
    return w - f32(lr) * upd, m, v


def ema_step(ema, w, d):
    """The EMA shadow from the weight BEFORE the step."""
    return ema - (1.0 - f32(d)) * (ema - w)


# The data of the kernel-level tests.  |g| >= 0.5 and |wd * w| <= 0.1: g' never cancels, so that no element sits where Adam's
# quotient g' / (|g'| + eps) magnifies a float32 rounding of g' (|g'| ~ eps).  wd = 0.05 makes a forgotten decay term visible.
KERNEL_WD = 0.05
KERNEL_HYPER = dict(lr=0.0094, d=0.999)


def kernel_data(n, seed):
    """(w, g, ema) float32 for one range."""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-2, 2, n).astype(np.float32)
    g = (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * (0.5 + np.abs(rng.randn(n)))).astype(np.float32)
    return w, g, (w * 0.5).astype(np.float32)


# (rule name, keyword arguments of the oracle and of the kernel wrapper) -- the oracle cases of the issue
RULES = [("sgd", dict(momentum=0.0, nesterov=False)), ("sgd", dict(momentum=0.9, nesterov=False)),
         ("sgd", dict(momentum=0.0, nesterov=True)), ("sgd", dict(momentum=0.9, nesterov=True)),
         ("adam", dict(wd_decoupled=0.0)), ("adam", dict(wd_decoupled=0.01))]


def two_steps(dtype, w, g, ema, rule, kw, wd=KERNEL_WD, scale=None, t0=0):
    """Two steps of `rule` from zero slots in `dtype`: the state [(w, slot a, slot b, ema)] after each."""
    w, g, ema = (np.asarray(x, dtype) for x in (w, g, ema))
    a, b = np.zeros_like(w), np.zeros_like(w)
    out = []
    for k in (1, 2):
        ema = ema_step(ema, w, KERNEL_HYPER["d"])
        if rule == "sgd":
            w, a = sgd_step(w, g, a, KERNEL_HYPER["lr"], wd=wd, scale=scale, **kw)
        else:
            w, a, b = adam_step(w, g, a, b, t0 + k, KERNEL_HYPER["lr"], wd=wd, scale=scale, **kw)
        out.append((w, a, b, ema))
    return out


# The sizes of the kernel-level GPU tests, so that the float32 check below runs on the very data they use.  The last is one full
# grid stride of 16-byte groups plus 259 AS THE LIBRARY HAS IT TODAY (a grid cap of 2048 workgroups of 256 lanes, four floats
# each); no device is at hand here to ask.  test_gpu_optimizer.py reads the stride from the library and asserts that its
# sizes are these: a change of the grid cap shows there as a failed assertion about THIS constant, which is then updated.
KERNEL_NS = (1, 3, 259, 100003, 2048 * 1024 + 259)


@pytest.mark.parametrize("case", range(len(KERNEL_NS)))
@pytest.mark.parametrize("rule,kw", RULES)
def test_float32_restatement_meets_the_bar_against_float64(case, rule, kw):
    """The seeds the GPU tests use (300 + case): float32 numpy alone stays inside rtol 1e-5 / atol 1e-6 of the float64 anchor
    on every output, so the bar asks the kernel for nothing float32 arithmetic cannot give."""
    w, g, ema = kernel_data(KERNEL_NS[case], 300 + case)
    for scale in (None, 0.5):
        lo, hi = two_steps(np.float32, w, g, ema, rule, kw, scale=scale), two_steps(np.float64, w, g, ema, rule, kw, scale=scale)
        for k, (s32, s64) in enumerate(zip(lo, hi)):
            for name, x, y in zip(("w", "a", "b", "ema"), s32, s64):
                assert x.dtype == np.float32 and y.dtype == np.float64
                err = np.abs(x - y) / (ATOL + RTOL * np.abs(y))
                assert err.max() <= 1.0, (name, k, float(err.max()))


def test_oracles_by_hand():
    one = lambda x: np.array([x], np.float64)
    # sgd: acc = 0.5 * 2 + 4 = 5; w = 1 - 0.25 * 5; nesterov: w = 1 - 0.25 * (4 + 0.5 * 5)
    w, acc = sgd_step(one(1), one(4), one(2), 0.25, momentum=0.5)
    assert w[0] == -0.25 and acc[0] == 5
    w, acc = sgd_step(one(1), one(4), one(2), 0.25, momentum=0.5, nesterov=True)
    assert w[0] == 1 - 0.25 * 6.5 and acc[0] == 5
    w, acc = sgd_step(one(1), one(4), None, 0.25, momentum=0.0, wd=0.5, scale=0.5)      # g' = 0.5 * (4 + 0.5 * 1)
    assert w[0] == 1 - 0.25 * 2.25 and acc is None
    # adam, t = 1 from zero moments: m^ = g, v^ = g^2 -> the step is lr * g / (|g| + eps), whatever the betas
    w, m, v = adam_step(one(1), one(-3), one(0), one(0), 1, 0.25, beta1=0.5, beta2=0.75, eps=1.0)
    assert m[0] == -1.5 and v[0] == 2.25 and np.isclose(w[0], 1 + 0.25 * 3 / 4, rtol=1e-15)
    w2, _, _ = adam_step(one(1), one(-3), one(0), one(0), 1, 0.25, beta1=0.5, beta2=0.75, eps=1.0, wd_decoupled=0.5)
    assert np.isclose(w2[0], w[0] - 0.25 * 0.5 * 1, rtol=1e-15)
    assert ema_step(one(2), one(4), 0.75)[0] == 2.5


def test_adam_oracle_agrees_with_torch():
    import torch
    rng = np.random.RandomState(0)
    w0, gs = rng.randn(50), [rng.randn(50) for _ in range(3)]
    for cls, kw, okw in ((torch.optim.Adam, dict(weight_decay=0.0), {}), (torch.optim.AdamW, dict(weight_decay=0.25), dict(wd_decoupled=0.25))):
        p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
        opt = cls([p], lr=0.125, betas=(0.5, 0.75), eps=2.0 ** -20, **kw)
        w, m, v = w0.copy(), np.zeros(50), np.zeros(50)
        for t, g in enumerate(gs, start=1):
            p.grad = torch.from_numpy(g.copy())
            opt.step()
            w, m, v = adam_step(w, g, m, v, t, 0.125, beta1=0.5, beta2=0.75, eps=2.0 ** -20, **okw)
        # torch divides sqrt(v) by sqrt(bc2) and applies the decay to w first: the same step in another order of roundings
        assert np.allclose(p.detach().numpy(), w, rtol=1e-12, atol=1e-12), cls.__name__


# ------------------------------------------------------------------------------------------------------ config
def opt(d):
    from multibox_amd.config import Cfg, optimizer, with_defaults
    return optimizer(with_defaults(Cfg(d)))


def test_config_defaults():
    assert opt({}) == {} and opt({"OPTIMIZER": None}) == {} and opt({"LEARNING_RATE_WARMUP_STEPS": 0}) == {}
    assert opt({"OPTIMIZER": "rmsprop", "RMSPROP_EPSILON": 0.1}) == {"optimizer": "rmsprop"}
    assert opt({"OPTIMIZER": "sgd"}) == {"optimizer": "sgd", "sgd_momentum": 0.9, "sgd_nesterov": False}
    assert opt({"OPTIMIZER": "sgd", "SGD_MOMENTUM": 0, "SGD_NESTEROV": True, "RMSPROP_MOMENTUM": 0.5}) == {
        "optimizer": "sgd", "sgd_momentum": 0.0, "sgd_nesterov": True}           # (RMSPROP_* sit in DEFAULTS: ignored)
    assert opt({"OPTIMIZER": "adam"}) == {"optimizer": "adam", "adam_beta1": 0.9, "adam_beta2": 0.999, "adam_epsilon": 1e-8}
    assert opt({"OPTIMIZER": "adamw", "ADAM_BETA1": 0.5, "ADAM_EPSILON": 1e-6, "LEARNING_RATE_WARMUP_STEPS": 500.0}) == {
        "optimizer": "adamw", "adam_beta1": 0.5, "adam_beta2": 0.999, "adam_epsilon": 1e-6, "adamw_weight_decay": 0.01,
        "lr_warmup_steps": 500}
    assert opt({"OPTIMIZER": "adamw", "ADAMW_WEIGHT_DECAY": 0})["adamw_weight_decay"] == 0.0
    assert opt({"LEARNING_RATE_WARMUP_STEPS": 7}) == {"lr_warmup_steps": 7}
    assert all(isinstance(v, float) for k, v in opt({"OPTIMIZER": "adamw", "ADAM_BETA1": 0}).items() if k != "optimizer")


def test_config_reads_yaml(tmp_path):
    from multibox_amd.config import optimizer, parse_config_file, with_defaults
    f = tmp_path / "c.yaml"
    f.write_text("OPTIMIZER: sgd\nSGD_NESTEROV: true\nLEARNING_RATE_WARMUP_STEPS: 100\n")
    assert optimizer(with_defaults(parse_config_file(str(f)))) == {"optimizer": "sgd", "sgd_momentum": 0.9, "sgd_nesterov": True,
                                                                   "lr_warmup_steps": 100}
    f.write_text("OPTIMIZER: adam\nADAM_BETA2: .nan\n")
    with pytest.raises(ValueError, match="ADAM_BETA2"):
        optimizer(with_defaults(parse_config_file(str(f))))


NOT_NUMBERS = [True, False, "0.5", [0.5], float("nan")]


@pytest.mark.parametrize("kind,key,bad", [
    ("sgd", "SGD_MOMENTUM", NOT_NUMBERS + [1, 1.5, -0.1]),
    ("sgd", "SGD_NESTEROV", [0, 1, 0.5, "true", [True], float("nan")]),
    ("adam", "ADAM_BETA1", NOT_NUMBERS + [1, 1.0, -1e-9]),
    ("adamw", "ADAM_BETA2", NOT_NUMBERS + [1, 2, -0.5]),
    ("adam", "ADAM_EPSILON", NOT_NUMBERS + [0, 0.0, -1e-8, 1e-60, float("inf"), 1e39]),     # 1e-60 is 0 as a float32, 1e39 inf
    ("adamw", "ADAMW_WEIGHT_DECAY", NOT_NUMBERS + [-0.01, float("inf"), 1e39]),
    ("sgd", "LEARNING_RATE_WARMUP_STEPS", [True, "10", [10], float("nan"), -1, 2.5, 2 ** 31]),
    (None, "LEARNING_RATE_WARMUP_STEPS", [False, -3, 0.5]),
    ("adam", "OPTIMIZER", [True, 1, "lamb", "SGD", ["sgd"], float("nan"), ""]),
])
def test_config_rejects(kind, key, bad):
    for value in bad:
        d = {} if kind is None else {"OPTIMIZER": kind}
        d[key] = value
        with pytest.raises(ValueError, match=key):
            opt(d)


@pytest.mark.parametrize("kind,foreign", [
    (None, ["SGD_MOMENTUM", "SGD_NESTEROV", "ADAM_BETA1", "ADAM_BETA2", "ADAM_EPSILON", "ADAMW_WEIGHT_DECAY"]),
    ("rmsprop", ["SGD_MOMENTUM", "ADAM_EPSILON", "ADAMW_WEIGHT_DECAY"]),
    ("sgd", ["ADAM_BETA1", "ADAM_BETA2", "ADAM_EPSILON", "ADAMW_WEIGHT_DECAY"]),
    ("adam", ["SGD_MOMENTUM", "SGD_NESTEROV", "ADAMW_WEIGHT_DECAY"]),
    ("adamw", ["SGD_MOMENTUM", "SGD_NESTEROV"]),
])
def test_config_names_a_foreign_key(kind, foreign):
    for key in foreign:
        d = {key: False if key == "SGD_NESTEROV" else 0.5}     # valid values under their own rule
        if kind is not None:
            d["OPTIMIZER"] = kind
        with pytest.raises(ValueError, match=key):
            opt(d)
        d[key] = None                                          # null = absent
        opt(d)


@pytest.mark.parametrize("kw,name", [
    (dict(optimizer="lamb"), "optimizer"), (dict(optimizer=None), "optimizer"),
    (dict(sgd_momentum=1.0), "sgd_momentum"), (dict(sgd_momentum=-0.1), "sgd_momentum"), (dict(sgd_momentum=True), "sgd_momentum"),
    (dict(adam_beta1=1), "adam_beta1"), (dict(adam_beta2=float("nan")), "adam_beta2"), (dict(adam_beta2="0.9"), "adam_beta2"),
    (dict(adam_epsilon=0), "adam_epsilon"), (dict(adam_epsilon=1e-60), "adam_epsilon"), (dict(adam_epsilon=float("inf")), "adam_epsilon"),
    (dict(adamw_weight_decay=-1e-3), "adamw_weight_decay"), (dict(adamw_weight_decay=1e39), "adamw_weight_decay"),
])
def test_trainer_arguments_are_checked_like_the_keys(kw, name):
    """What Trainer.__init__ calls before it allocates anything: a Trainer built by hand is held to the config's ranges."""
    from multibox_amd import config, trainer
    assert trainer.check_optimizer_args is config.check_optimizer_args
    with pytest.raises(ValueError, match=name):
        config.check_optimizer_args(**dict(dict(optimizer="adamw"), **kw))
    for kind in config.OPTIMIZERS:
        config.check_optimizer_args(kind)
        config.check_optimizer_args(kind, 0, 0.0, 0.5, 1e-3, 0)
    assert not hasattr(trainer, "OPTIMIZERS")                  # one tuple, in config


# ------------------------------------------------------------------------------------------------------ warm-up
def test_warmup_factor_and_learning_rate():
    from multibox_amd.trainer import learning_rate, warmup_factor
    assert warmup_factor(0, 100) == 0.01 and warmup_factor(98, 100) == 0.99
    assert warmup_factor(99, 100) == 1.0 and warmup_factor(100, 100) == 1.0 and warmup_factor(10 ** 6, 100) == 1.0
    assert warmup_factor(0, 1) == 1.0
    for off in (0, None):
        assert warmup_factor(0, off) == 1.0 and warmup_factor(12345, off) == 1.0
    # learning_rate(): signature and results as before (tf.train.exponential_decay)
    import inspect
    assert list(inspect.signature(learning_rate).parameters) == ["step", "lr0", "dsteps", "factor", "staircase"]
    assert learning_rate(0, 0.01, 7116, 0.94) == 0.01 and learning_rate(7115, 0.01, 7116, 0.94) == 0.01
    assert learning_rate(7116, 0.01, 7116, 0.94) == 0.01 * 0.94 and learning_rate(3 * 7116 + 5, 0.01, 7116, 0.94) == 0.01 * 0.94 ** 3
    assert learning_rate(3558, 0.01, 7116, 0.94, staircase=False) == 0.01 * 0.94 ** 0.5


def test_trainer_takes_the_keys():
    import inspect
    from multibox_amd.trainer import Trainer
    p = inspect.signature(Trainer.__init__).parameters
    want = dict(optimizer="rmsprop", sgd_momentum=0.9, sgd_nesterov=False, adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8,
                adamw_weight_decay=0.01, lr_warmup_steps=0)
    assert {k: p[k].default for k in want} == want
    # every key config.optimizer can return is one of them
    full = opt({"OPTIMIZER": "adamw", "LEARNING_RATE_WARMUP_STEPS": 3})
    full.update(opt({"OPTIMIZER": "sgd"}))
    assert set(full) == set(want)


# ------------------------------------------------------------------------------------------------------ C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


def test_signatures(lib):
    from multibox_amd import _lib
    P, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_int64
    assert _lib._SIGS["mbx_sgd_ema_step"] == (I, [P, P, P, P, P, L, F, F, I, F, F, I, P, P, I, P])
    assert _lib._SIGS["mbx_adam_ema_step"] == (I, [P, P, P, P, P, P, L, F, F, F, F, F, F, L, P, F, I, P, P, I, P])
    for name in ("mbx_sgd_ema_step", "mbx_adam_ema_step"):
        fn = getattr(lib, name)
        assert fn.restype is I and list(fn.argtypes) == _lib._SIGS[name][1]
    assert lib.mbx_version() >= 101


SGD_ARGS = (("w", 0x10000), ("g", 0x10000), ("mom", 0x10000), ("ema", 0x10000), ("wb", 0x10000), ("n", 8), ("lr", 0.01), ("momentum", 0.9),
            ("nesterov", 0), ("wd", 4e-5), ("d", 0.999), ("on", 1), ("reg", None), ("ctl", None), ("clipped", 0), ("stream", None))
ADAM_ARGS = (("w", 0x10000), ("g", 0x10000), ("m", 0x10000), ("v", 0x10000), ("ema", 0x10000), ("wb", 0x10000), ("n", 8), ("lr", 0.01),
             ("beta1", 0.9), ("beta2", 0.999), ("eps", 1e-8), ("wd", 4e-5), ("wdd", 0.0), ("calls", 0), ("skipped", None), ("d", 0.999),
             ("on", 1), ("reg", None), ("ctl", None), ("clipped", 0), ("stream", None))
NAN, INF = float("nan"), float("inf")


def test_entry_points_reject_bad_arguments(lib):
    """Pointers here are made-up addresses: every call must be refused before anything is launched or read."""
    def refused(fn, table, **kw):
        assert not set(kw) - {k for k, _ in table}, kw
        return fn(*[kw.get(k, d) for k, d in table]) == INVALID
    sgd = lambda **kw: refused(lib.mbx_sgd_ema_step, SGD_ARGS, **kw)
    adam = lambda **kw: refused(lib.mbx_adam_ema_step, ADAM_ARGS, **kw)
    for both in (sgd, adam):
        assert both(n=-1) and both(n=-2 ** 40)
        assert both(w=None) and both(g=None)
        assert both(wd=-1e-9) and both(wd=NAN)
        assert both(clipped=1)                                 # clipped without its block
        assert both(clipped=1, ctl=None, on=0)
    assert sgd(momentum=0.0)                                   # a slot without momentum
    assert sgd(mom=None)                                       # momentum without its slot
    assert sgd(mom=None, on=0)                                 # ... frozen ranges too
    for bad in (1.0, 1.5, -0.1, NAN, INF):
        assert sgd(momentum=bad), bad
        assert adam(beta1=bad) and adam(beta2=bad), bad
    assert adam(m=None) and adam(v=None)
    for bad in (0.0, -1e-8, NAN):
        assert adam(eps=bad), bad
    assert adam(wdd=-0.01) and adam(wdd=NAN)
    assert adam(calls=-1)
    # what is NOT an error is refused by none of the checks: n = 0 returns MBX_OK without a launch
    assert lib.mbx_sgd_ema_step(*[dict(SGD_ARGS, n=0)[k] for k, _ in SGD_ARGS]) == 0
    assert lib.mbx_sgd_ema_step(*[dict(SGD_ARGS, n=0, mom=None, momentum=0.0, g=None, on=0)[k] for k, _ in SGD_ARGS]) == 0
    assert lib.mbx_adam_ema_step(*[dict(ADAM_ARGS, n=0)[k] for k, _ in ADAM_ARGS]) == 0
    assert lib.mbx_adam_ema_step(*[dict(ADAM_ARGS, n=0, g=None, m=None, v=None, on=0, clipped=1, ctl=0x10000)[k] for k, _ in ADAM_ARGS]) == 0
