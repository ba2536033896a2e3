"""LAYERWISE_TRUST / LAYERWISE_TRUST_COEFF without a device: the config keys, the Trainer's keyword arguments, the chunk plan
(host code) against the restatement of tests/trust_oracle.py byte for byte, the ctypes signatures and the argument checks of the
device entry points (they come before any launch), and the float32 restatement of LARS and LAMB against the float64 oracle
on the very data of tests/test_gpu_trust.py.

Bars (the GPU tests use the same).  Ratios: rtol 1e-6 -- the kernel rounds g' (or u) to float32 before widening where the
float64 oracle does not, at most 2^-24 relative per element and so on the norm, and the result is rounded to float32 once
more: 1.2e-7 in all, 8x headroom.  Updates: rtol 1e-5 / atol 1e-6, the optimiser bar of tests/test_optimizer_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

from tests import test_optimizer_cpu as OC
from tests import trust_oracle as TO

INVALID = OC.INVALID
RATIO_RTOL = 1e-6
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------------ config
def trust(d):
    from multibox_amd.config import Cfg, layerwise_trust, with_defaults
    return layerwise_trust(with_defaults(Cfg(d)))


def test_config_defaults():
    assert trust({}) is None and trust({"LAYERWISE_TRUST": None}) is None and trust({"LAYERWISE_TRUST": False}) is None
    assert trust({"OPTIMIZER": "sgd"}) is None and trust({"OPTIMIZER": "adam", "LAYERWISE_TRUST": False}) is None
    assert trust({"LAYERWISE_TRUST": False, "LAYERWISE_TRUST_COEFF": None}) is None
    # off needs no rule: the switch alone decides
    assert trust({"OPTIMIZER": "rmsprop", "LAYERWISE_TRUST": False}) is None
    assert trust({"OPTIMIZER": "sgd", "LAYERWISE_TRUST": True}) == {"layerwise_trust": True, "trust_coeff": 0.001}
    assert trust({"OPTIMIZER": "adam", "LAYERWISE_TRUST": True}) == {"layerwise_trust": True, "trust_coeff": 1.0}
    assert trust({"OPTIMIZER": "adamw", "LAYERWISE_TRUST": True}) == {"layerwise_trust": True, "trust_coeff": 1.0}
    got = trust({"OPTIMIZER": "adamw", "LAYERWISE_TRUST": True, "LAYERWISE_TRUST_COEFF": 2})
    assert got == {"layerwise_trust": True, "trust_coeff": 2.0} and isinstance(got["trust_coeff"], float)
    assert trust({"OPTIMIZER": "sgd", "LAYERWISE_TRUST": True, "LAYERWISE_TRUST_COEFF": 0.02})["trust_coeff"] == 0.02


def test_config_reads_yaml(tmp_path):
    from multibox_amd.config import layerwise_trust, optimizer, parse_config_file, with_defaults
    f = tmp_path / "c.yaml"
    f.write_text("OPTIMIZER: sgd\nLAYERWISE_TRUST: true\nLAYERWISE_TRUST_COEFF: 0.002\n")
    cfg = with_defaults(parse_config_file(str(f)))
    assert layerwise_trust(cfg) == {"layerwise_trust": True, "trust_coeff": 0.002}
    assert optimizer(cfg) == {"optimizer": "sgd", "sgd_momentum": 0.9, "sgd_nesterov": False}      # the rule's keys are its own
    f.write_text("OPTIMIZER: adamw\nLAYERWISE_TRUST: true\n")
    assert layerwise_trust(with_defaults(parse_config_file(str(f)))) == {"layerwise_trust": True, "trust_coeff": 1.0}
    f.write_text("OPTIMIZER: adam\nLAYERWISE_TRUST: true\nLAYERWISE_TRUST_COEFF: .nan\n")
    with pytest.raises(ValueError, match="LAYERWISE_TRUST_COEFF"):
        layerwise_trust(with_defaults(parse_config_file(str(f))))
    f.write_text("OPTIMIZER: adam\nLAYERWISE_TRUST: yes please\n")
    with pytest.raises(ValueError, match="LAYERWISE_TRUST"):
        layerwise_trust(with_defaults(parse_config_file(str(f))))


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_config_rejects(kind):
    for bad in (0, 1, 0.5, "true", "false", [True], NAN):
        with pytest.raises(ValueError, match="LAYERWISE_TRUST must"):
            trust({"OPTIMIZER": kind, "LAYERWISE_TRUST": bad})
    # 1e-60 is 0 as a float32, 1e39 inf
    for bad in (True, False, "0.5", [0.5], NAN, 0, 0.0, -0.001, INF, 1e-60, 1e39):
        with pytest.raises(ValueError, match="LAYERWISE_TRUST_COEFF"):
            trust({"OPTIMIZER": kind, "LAYERWISE_TRUST": True, "LAYERWISE_TRUST_COEFF": bad})
    for switch in ({}, {"LAYERWISE_TRUST": None}, {"LAYERWISE_TRUST": False}):      # the coefficient without the switch
        with pytest.raises(ValueError, match="LAYERWISE_TRUST_COEFF"):
            trust(dict(switch, OPTIMIZER=kind, LAYERWISE_TRUST_COEFF=0.5))


@pytest.mark.parametrize("d", [{}, {"OPTIMIZER": None}, {"OPTIMIZER": "rmsprop"}])
def test_config_names_both_keys_under_rmsprop(d):
    with pytest.raises(ValueError) as e:
        trust(dict(d, LAYERWISE_TRUST=True))
    assert "LAYERWISE_TRUST" in str(e.value) and "OPTIMIZER" in str(e.value)


def test_optimizer_keys_are_untouched():
    """config.optimizer() neither reads nor returns the new keys: the set test_optimizer_cpu.test_trainer_takes_the_keys pins."""
    want = {"optimizer", "sgd_momentum", "sgd_nesterov", "adam_beta1", "adam_beta2", "adam_epsilon", "adamw_weight_decay", "lr_warmup_steps"}
    extra = {"LAYERWISE_TRUST": True, "LAYERWISE_TRUST_COEFF": 0.5}
    full = OC.opt(dict(extra, OPTIMIZER="adamw", LEARNING_RATE_WARMUP_STEPS=3))
    full.update(OC.opt(dict(extra, OPTIMIZER="sgd")))
    assert set(full) == want
    assert OC.opt(dict(extra, OPTIMIZER="sgd")) == OC.opt({"OPTIMIZER": "sgd"})
    with pytest.raises(ValueError, match="OPTIMIZER"):
        OC.opt({"OPTIMIZER": "lamb"})                            # not a rule: sgd / adam + LAYERWISE_TRUST


def test_trainer_takes_the_keys_last():
    import inspect
    from multibox_amd import config, trainer
    names = list(inspect.signature(trainer.Trainer.__init__).parameters)
    assert names[-2:] == ["layerwise_trust", "trust_coeff"] and names[-3] == "atss_topk"
    p = inspect.signature(trainer.Trainer.__init__).parameters
    assert p["layerwise_trust"].default is False and p["trust_coeff"].default is None
    assert list(inspect.signature(config.check_optimizer_args).parameters) == [
        "optimizer", "sgd_momentum", "adam_beta1", "adam_beta2", "adam_epsilon", "adamw_weight_decay"]
    assert set(trust({"OPTIMIZER": "sgd", "LAYERWISE_TRUST": True})) <= set(names)


def test_trainer_arguments_are_checked_like_the_keys():
    from multibox_amd.config import check_trust_args
    assert check_trust_args("rmsprop") is None and check_trust_args("sgd", False, None) is None
    assert check_trust_args("sgd", True) == 0.001 and check_trust_args("adam", True) == 1.0 and check_trust_args("adamw", True, 3) == 3.0
    with pytest.raises(ValueError, match="layerwise_trust"):
        check_trust_args("rmsprop", True)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="layerwise_trust"):
            check_trust_args("sgd", bad)
    for bad in (True, "1", [1.0], NAN, 0, -1.0, INF, 1e-60, 1e39):
        with pytest.raises(ValueError, match="trust_coeff"):
            check_trust_args("adam", True, bad)
    with pytest.raises(ValueError, match="trust_coeff"):
        check_trust_args("adam", False, 0.5)


# ------------------------------------------------------------------------------------------------------ the plan
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


def test_chunk_size(lib):
    CH = int(lib.mbx_trust_chunk_elems())
    assert CH >= 1024 and CH % 1024 == 0 and CH & (CH - 1) == 0
    assert lib.mbx_version() >= 102


def library_plan(lib, bounds, adapt):
    from multibox_amd import _lib
    nv = len(bounds) - 1
    b = (C.c_int64 * (nv + 1))(*[int(x) for x in bounds])
    a = (C.c_int32 * nv)(*[int(x) for x in adapt])
    nc = int(lib.mbx_trust_plan_count(b, nv))
    assert nc > 0
    chunks, vars_ = (_lib.TrustChunk * (nc + 1))(), (_lib.TrustVar * (nv + 1))()
    chunks[nc].len = vars_[nv].pad = -77                          # canaries behind both images
    assert lib.mbx_trust_plan(b, a, nv, chunks, vars_) == 0
    assert chunks[nc].len == -77 and vars_[nv].pad == -77
    assert C.sizeof(_lib.TrustChunk) == 16 and C.sizeof(_lib.TrustVar) == 16
    return nc, bytes(chunks)[:16 * nc], bytes(vars_)[:16 * nv]


def partitions(CH):
    rng = np.random.RandomState(77)
    return {"one of 1": TO.bounds_of([1]),
            "1 3 4 5 259": TO.bounds_of([1, 3, 4, 5, 259]),
            "exactly CH": TO.bounds_of([CH]),
            "CH + 1": TO.bounds_of([CH + 1]),
            "2 CH + 7 from 3": TO.bounds_of([2 * CH + 7], start=3),
            "bound on a multiple of CH": TO.bounds_of([CH - 5, 5, 7, 2 * CH - 7, 11]),
            "600 random": TO.bounds_of(rng.randint(1, 3 * CH + 1, 600).tolist())}


@pytest.mark.parametrize("which", range(7))
def test_plan_is_the_restatement_byte_for_byte(lib, which):
    CH = int(lib.mbx_trust_chunk_elems())
    name, bounds = sorted(partitions(CH).items())[which]
    adapt = [(i * 7 + 1) % 3 != 0 for i in range(len(bounds) - 1)]
    nc, cbytes, vbytes = library_plan(lib, bounds, adapt)
    want_c, want_v = TO.plan_images(bounds, adapt, CH)
    assert cbytes == want_c and vbytes == want_v, name
    chunks = np.frombuffer(cbytes, TO.CHUNK_DTYPE)
    vars_ = np.frombuffer(vbytes, TO.VAR_DTYPE)
    assert nc == len(chunks) == int(vars_["n_chunks"].sum())
    # the chunks tile the range in order, none is empty or longer than CH, each lies in one variable and in one grid cell
    assert chunks["lo"][0] == 0 and (chunks["lo"][1:] == chunks["lo"][:-1] + chunks["len"][:-1]).all()
    assert chunks["lo"][-1] + chunks["len"][-1] == bounds[-1]
    assert (chunks["len"] >= 1).all() and (chunks["len"] <= CH).all()
    assert (chunks["lo"] >= bounds[chunks["var"]]).all() and (chunks["lo"] + chunks["len"] <= bounds[chunks["var"] + 1]).all()
    assert (chunks["lo"] // CH == (chunks["lo"] + chunks["len"] - 1) // CH).all()
    # a chunk starts on the grid or at a variable bound
    assert all(lo % CH == 0 or lo == bounds[v] for lo, v in zip(chunks["lo"], chunks["var"]))
    for i, v in enumerate(vars_):
        own = chunks[v["first_chunk"]:v["first_chunk"] + v["n_chunks"]]
        assert (own["var"] == i).all() and own["len"].sum() == bounds[i + 1] - bounds[i] and v["adapt"] == int(adapt[i])
    if name == "bound on a multiple of CH":
        assert CH in bounds and 3 * CH in bounds and nc == 6
    if name == "2 CH + 7 from 3":
        assert [tuple(c) for c in chunks] == [(0, 3, 0), (3, CH - 3, 1), (CH, CH, 1), (2 * CH, 10, 1)]


def test_plan_refuses_bad_arguments(lib):
    from multibox_amd import _lib
    arr = lambda xs: (C.c_int64 * len(xs))(*xs)
    adapt, chunks, vars_ = (C.c_int32 * 4)(1, 1, 1, 1), (_lib.TrustChunk * 16)(), (_lib.TrustVar * 4)()
    good = arr([0, 5, 9])
    assert lib.mbx_trust_plan_count(good, 2) == 2 and lib.mbx_trust_plan(good, adapt, 2, chunks, vars_) == 0
    for bounds, nv in ((good, 0), (good, -1), (None, 2), (arr([1, 5, 9]), 2), (arr([0, 5, 5]), 2), (arr([0, 5, 4]), 2),
                       (arr([0, 0, 4]), 2), (arr([0, -3, 4]), 2), (arr([-1, 5, 9]), 2)):
        assert lib.mbx_trust_plan_count(bounds, nv) == 0, (list(bounds) if bounds else None, nv)
        assert lib.mbx_trust_plan(bounds, adapt, nv, chunks, vars_) == INVALID
    assert lib.mbx_trust_plan(good, None, 2, chunks, vars_) == INVALID
    assert lib.mbx_trust_plan(good, adapt, 2, None, vars_) == INVALID
    assert lib.mbx_trust_plan(good, adapt, 2, chunks, None) == INVALID


# ------------------------------------------------------------------------------------------------------ C ABI
def test_signatures(lib):
    from multibox_amd import _lib
    P, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_int64
    want = {"mbx_trust_chunk_elems": (L, []),
            "mbx_trust_plan_count": (L, [P, L]),
            "mbx_trust_plan": (I, [P, P, L, P, P]),
            "mbx_trust_norms_sgd": (I, [P, P, P, L, F, P, P, I, P]),
            "mbx_trust_moments_adam": (I, [P, P, P, P, P, L, F, F, F, F, F, L, P, P, P, I, P]),
            "mbx_trust_ratios": (I, [P, P, L, F, P, P, P]),
            # the twins' arguments, then chunks, n_chunks, ratio in front of the stream
            "mbx_sgd_ema_step_trust": (I, _lib._SIGS["mbx_sgd_ema_step"][1][:-1] + [P, L, P, P]),
            "mbx_adam_ema_step_trust": (I, _lib._SIGS["mbx_adam_ema_step"][1][:-1] + [P, L, P, P])}
    for name, sig in want.items():
        assert _lib._SIGS[name] == sig, name
        fn = getattr(lib, name)
        assert fn.restype is sig[0] and list(fn.argtypes) == sig[1]


A = 0x10000                                                    # a made-up, aligned address
TRUST_TAIL = (("chunks", A), ("n_chunks", 3), ("ratio", A), ("stream", None))
SGD_ARGS = OC.SGD_ARGS[:-1] + TRUST_TAIL
ADAM_ARGS = OC.ADAM_ARGS[:-1] + TRUST_TAIL
NORMS_ARGS = (("w", A), ("g", A), ("chunks", A), ("n_chunks", 3), ("wd", 4e-5), ("partials", A), ("ctl", None), ("clipped", 0), ("stream", None))
MOMENTS_ARGS = (("w", A), ("g", A), ("m", A), ("v", A), ("chunks", A), ("n_chunks", 3), ("beta1", 0.9), ("beta2", 0.999), ("eps", 1e-8),
                ("wd", 4e-5), ("wdd", 0.0), ("calls", 0), ("skipped", None), ("partials", A), ("ctl", None), ("clipped", 0), ("stream", None))
RATIOS_ARGS = (("partials", A), ("vars", A), ("n_vars", 2), ("coeff", 0.5), ("ratio", A), ("ctl", None), ("stream", None))


def test_entry_points_reject_bad_arguments(lib):
    """Pointers here are made-up addresses: every call must be refused before anything is launched or read."""
    def refused(fn, table, **kw):
        assert not set(kw) - {k for k, _ in table}, kw
        return fn(*[kw.get(k, d) for k, d in table]) == INVALID
    sgd = lambda **kw: refused(lib.mbx_sgd_ema_step_trust, SGD_ARGS, **kw)
    adam = lambda **kw: refused(lib.mbx_adam_ema_step_trust, ADAM_ARGS, **kw)
    norms = lambda **kw: refused(lib.mbx_trust_norms_sgd, NORMS_ARGS, **kw)
    moments = lambda **kw: refused(lib.mbx_trust_moments_adam, MOMENTS_ARGS, **kw)
    ratios = lambda **kw: refused(lib.mbx_trust_ratios, RATIOS_ARGS, **kw)
    # what the twins refuse
    for both in (sgd, adam):
        assert both(n=-1) and both(n=-2 ** 40)
        assert both(w=None) and both(g=None)
        assert both(wd=-1e-9) and both(wd=NAN)
        assert both(clipped=1) and both(clipped=1, ctl=None, on=0)
        assert both(chunks=None) and both(chunks=A + 4) and both(ratio=None) and both(n_chunks=-1) and both(n_chunks=2 ** 31)
    assert sgd(momentum=0.0) and sgd(mom=None) and sgd(mom=None, on=0)
    for bad in (1.0, 1.5, -0.1, NAN, INF):
        assert sgd(momentum=bad), bad
        assert adam(beta1=bad) and adam(beta2=bad) and moments(beta1=bad) and moments(beta2=bad), bad
    assert adam(m=None) and adam(v=None) and moments(m=None) and moments(v=None)
    for bad in (0.0, -1e-8, NAN):
        assert adam(eps=bad) and moments(eps=bad), bad
    assert adam(wdd=-0.01) and adam(wdd=NAN) and adam(calls=-1)
    assert moments(wdd=-0.01) and moments(wdd=NAN) and moments(calls=-1)
    # the norm passes
    for both in (norms, moments):
        assert both(w=None) and both(g=None) and both(chunks=None) and both(chunks=A + 4)
        assert both(n_chunks=0) and both(n_chunks=-1) and both(n_chunks=2 ** 31)
        assert both(wd=-1e-9) and both(wd=NAN)
        assert both(partials=None) and both(partials=A + 4)
        assert both(clipped=1)
    # the ratios
    assert ratios(partials=None) and ratios(partials=A + 4) and ratios(vars=None) and ratios(ratio=None)
    assert ratios(n_vars=0) and ratios(n_vars=-1) and ratios(n_vars=2 ** 31)
    for bad in (0.0, -0.5, NAN, INF):
        assert ratios(coeff=bad), bad
    # what is NOT an error is refused by none of the checks: an empty range returns MBX_OK without a launch
    assert lib.mbx_sgd_ema_step_trust(*[dict(SGD_ARGS, n=0)[k] for k, _ in SGD_ARGS]) == 0
    assert lib.mbx_adam_ema_step_trust(*[dict(ADAM_ARGS, n=0)[k] for k, _ in ADAM_ARGS]) == 0
    assert lib.mbx_sgd_ema_step_trust(*[dict(SGD_ARGS, n_chunks=0)[k] for k, _ in SGD_ARGS]) == 0
    assert lib.mbx_adam_ema_step_trust(*[dict(ADAM_ARGS, n_chunks=0, clipped=1, ctl=A)[k] for k, _ in ADAM_ARGS]) == 0


# ------------------------------------------------------------------------------------------------------ oracle
def test_oracle_by_hand():
    one = lambda *x: np.array(x, np.float64)
    bounds, w, g = np.array([0, 2, 3]), one(3, 4, 2), one(0.6, 0.8, 5)
    # ||w|| = 5, ||g|| = 1 -> r = 0.5 * 5; the second variable does not adapt
    assert TO.ratios(w, g, bounds, [1, 0], 0.5).tolist() == [2.5, 1.0]
    assert TO.ratios(w * 0, g, bounds, [1, 1], 0.5).tolist() == [1.0, 1.0]
    assert TO.ratios(w, g * 0, bounds, [1, 1], 0.5).tolist() == [1.0, 1.0]
    assert TO.ratios(w.astype(np.float32), g.astype(np.float32), bounds, [1, 1], 0.5).dtype == np.float32
    # LARS: acc = 0.5 * acc + r g; w -= 0.25 * acc
    w1, acc, r = TO.lars_step(w, g, one(2, 2, 2), bounds, [1, 0], 0.5, 0.25, momentum=0.5)
    assert r.tolist() == [2.5, 1.0] and acc.tolist() == [1 + 1.5, 1 + 2.0, 1 + 5.0] and w1.tolist() == [3 - 0.625, 4 - 0.75, 2 - 1.5]
    # LAMB, t = 1 from zero moments, eps = 1: u = g / (|g| + 1)
    w1, m, v, r = TO.lamb_step(w, one(1, -1, 3), one(0, 0, 0), one(0, 0, 0), 1, bounds, [1, 0], 0.5, 0.25, beta1=0.5, beta2=0.75, eps=1.0)
    u = one(0.5, -0.5, 0.75)
    assert np.allclose(r, [0.5 * 5 / np.sqrt(0.5), 1.0], rtol=1e-15) and np.allclose(w1, w - 0.25 * np.repeat(r, [2, 1]) * u, rtol=1e-15)
    # with every ratio 1 both are the plain rules
    w2, acc2, _ = TO.lars_step(w, g, one(2, 2, 2), bounds, [0, 0], 0.5, 0.25, momentum=0.5, nesterov=True, wd=0.125)
    w3, acc3 = OC.sgd_step(w, g, one(2, 2, 2), 0.25, momentum=0.5, nesterov=True, wd=0.125)
    assert w2.tolist() == w3.tolist() and acc2.tolist() == acc3.tolist()
    w2, _, _, _ = TO.lamb_step(w, g, one(1, 1, 1), one(2, 2, 2), 3, bounds, [0, 0], 0.5, 0.25, wd=0.125, wd_decoupled=0.5)
    w3, _, _ = OC.adam_step(w, g, one(1, 1, 1), one(2, 2, 2), 3, 0.25, wd=0.125, wd_decoupled=0.5)
    assert np.allclose(w2, w3, rtol=1e-15)


@pytest.mark.parametrize("rule,kw", TO.CASES)
def test_float32_restatement_meets_the_bars_against_float64(lib, rule, kw):
    """On SMALL with the seed the GPU tests use: float32 numpy alone stays inside both bars, so they ask the kernels for
    nothing float32 arithmetic cannot give."""
    CH = int(lib.mbx_trust_chunk_elems())
    bounds, adapt = TO.small(CH)
    w, g, ema = TO.small_data(CH)
    for scale in (None, 0.5):
        lo = TO.two_steps(np.float32, w, g, ema, bounds, adapt, rule, kw, scale=scale)
        hi = TO.two_steps(np.float64, w, g, ema, bounds, adapt, rule, kw, scale=scale)
        for k, (s32, s64) in enumerate(zip(lo, hi)):
            for name, x, y in zip(("w", "a", "b", "ema"), s32, s64):
                assert x.dtype == np.float32 and y.dtype == np.float64
                err = np.abs(x - y) / (OC.ATOL + OC.RTOL * np.abs(y))
                assert err.max() <= 1.0, (name, k, float(err.max()))
            r32, r64 = s32[4], s64[4]
            assert r32.dtype == np.float32 and np.allclose(r32, r64, rtol=RATIO_RTOL, atol=0), (k, r32, r64)
            # (the zero-w variable has moved by the second step: ratio 1 made its first step the plain rule's)
            assert (r64[TO.ZERO_W] == 1.0) == (k == 0) and (r64[-2:] == 1.0).all() and (r64[:TO.ZERO_W] != 1.0).all()
        assert np.abs(hi[1][0] - w).max() > 1e-3               # the two steps moved the weights
