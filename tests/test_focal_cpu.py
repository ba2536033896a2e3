"""The focal loss on the confidence term (mbx_loss_fwd_bwd_focal), the parts that need no GPU: the config keys, the numpy
restatement the GPU tests compare against (tests/focal_oracle.py) -- anchored to oracle.ref_numpy at gamma = 0, its
gradient checked by central differences, its bars shown to hold for a float32 evaluation of the same formulas -- the
MultiboxLoss keywords and the ctypes table."""
import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import focal_oracle as FO
from tests import mined_oracle as MO
from tests.test_gpu_loss_focal import SHAPES, make_case

G_KEY, A_KEY = "LOSS_FOCAL_GAMMA", "LOSS_FOCAL_ALPHA"


# ------------------------------------------------------------------------------------------------- config keys
@pytest.mark.parametrize("cfg,want", [
    ({}, None),
    ({G_KEY: None}, None),
    ({G_KEY: None, A_KEY: None}, None),
    ({G_KEY: 2}, (2.0, None)),
    ({G_KEY: 2.0, A_KEY: None}, (2.0, None)),
    ({G_KEY: 0}, (0.0, None)),
    ({G_KEY: 10}, (10.0, None)),
    ({G_KEY: 0.5, A_KEY: 0.25}, (0.5, 0.25)),
    ({G_KEY: 2, A_KEY: 0.999}, (2.0, 0.999)),
])
def test_focal_loss_accepts(cfg, want):
    from multibox_amd.config import Cfg, focal_loss, with_defaults
    assert focal_loss(Cfg(cfg)) == want
    got = focal_loss(with_defaults(Cfg(cfg)))                 # the defaults switch nothing on
    assert got == want and (got is None or (type(got[0]) is float and type(got[1]) in (float, type(None))))


@pytest.mark.parametrize("cfg,key", [({G_KEY: v}, G_KEY) for v in (-0.1, 10.5, True, False, "2", [2], float("nan"), float("inf"))]
                         + [({G_KEY: 2, A_KEY: v}, A_KEY) for v in (0, 1, 0.0, 1.0, -0.25, 1.5, True, False, "0.25", [0.25],
                                                                     float("nan"), float("inf"))]
                         + [({A_KEY: 0.25}, A_KEY), ({G_KEY: None, A_KEY: 0.25}, A_KEY)])
def test_focal_loss_rejects(cfg, key):
    from multibox_amd.config import Cfg, focal_loss
    with pytest.raises(ValueError, match=key):
        focal_loss(Cfg(cfg))


def test_the_focal_keys_compose_with_mining_and_threshold_matching():
    from multibox_amd.config import Cfg, focal_loss, match_iou_threshold, negative_mining
    cfg = Cfg({G_KEY: 2, A_KEY: 0.25, "LOSS_NEG_PER_POS": 3, "LOSS_MATCH_IOU_THRESHOLD": 0.4})
    assert focal_loss(cfg) == (2.0, 0.25) and negative_mining(cfg) == (3, 0) and match_iou_threshold(cfg) == 0.4
    assert focal_loss(Cfg({"LOSS_NEG_PER_POS": 3, "LOSS_MATCH_IOU_THRESHOLD": 0.4})) is None
    assert negative_mining(Cfg({G_KEY: 2})) is None and match_iou_threshold(Cfg({G_KEY: 2})) is None


def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch):
    import torch
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\n%s: 2\n%s: 1.5\n" % (G_KEY, A_KEY))

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match=A_KEY):
        train.main()


# ------------------------------------------------------------------------------- the oracle: anchored to ref_numpy
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("conf_is_logit", [1, 0])
def test_gamma_zero_unit_weights_is_ref_numpy_bit_for_bit(B, P, G, conf_is_logit):
    c = make_case(B, P, G)
    x = c["z"] if conf_is_logit else c["x"]
    zero = np.zeros((P, 4), np.float32)
    out = FO.focal_loss(c["dec"], x, conf_is_logit, c["gt"], c["match"], 1000.0, 0.0, 1.0, 1.0, 0, 0)
    ref = R.add_loss(c["dec"], R.sigmoid_f32(x) if conf_is_logit else x, c["gt"], c["n_pos"], zero, 1000.0, match=c["match"])
    assert np.array_equal(out["n_neg"], P - c["n_pos"]) and np.array_equal(out["mask"], c["match"] < 0)
    assert out["loc_loss"].tobytes() == ref["loc_loss"].tobytes()
    assert out["conf_loss"].dtype == np.float32 and out["conf_loss"].tobytes() == ref["conf_loss"].tobytes()
    if conf_is_logit:
        dl, dz = R.add_loss_grads(c["dec"], x, c["gt"], zero, 1000.0, c["match"])
        assert out["d_locs"].tobytes() == dl.tobytes() and out["d_conf_in"].tobytes() == dz.tobytes()
    for neg_per_pos, min_neg in ((3, 0), (3, 5), (3, P)):
        out = FO.focal_loss(c["dec"], x, conf_is_logit, c["gt"], c["match"], 1000.0, 0.0, 1.0, 1.0, neg_per_pos, min_neg)
        ref = MO.mined_loss(c["dec"], x, conf_is_logit, c["gt"], c["match"], 1000.0, neg_per_pos, min_neg)
        assert np.array_equal(out["mask"], ref["mask"]) and np.array_equal(out["n_neg"], ref["n_neg"])
        for k in ("loc_loss", "conf_loss", "d_locs", "d_conf_in"):
            assert np.asarray(out[k]).dtype == np.float32 and np.asarray(out[k]).tobytes() == np.asarray(ref[k]).tobytes(), k


def test_the_weights_scale_each_side():
    c = make_case(4, 70, 5)
    one = FO.focal_loss(c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, 2.0, 1.0, 1.0, 0, 0)
    pos_only = FO.focal_loss(c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, 2.0, 0.25, 0.0, 0, 0)
    neg_only = FO.focal_loss(c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, 2.0, 0.0, 0.75, 0, 0)
    pos = c["match"] >= 0
    assert np.allclose(pos_only["d_conf_in"][pos], 0.25 * one["d_conf_in"][pos], rtol=1e-6) and not pos_only["d_conf_in"][~pos].any()
    assert np.allclose(neg_only["d_conf_in"][~pos], 0.75 * one["d_conf_in"][~pos], rtol=1e-6) and not neg_only["d_conf_in"][pos].any()
    both = FO.focal_loss(c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, 2.0, 0.25, 0.75, 0, 0)
    assert np.isclose(float(both["conf_loss"]), float(pos_only["conf_loss"]) + float(neg_only["conf_loss"]), rtol=1e-6)
    # gamma > 0 takes weight off the well-classified: every term shrinks, none changes sign
    assert 0 < float(one["conf_loss"]) < float(FO.focal_loss(c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, 0.0, 1.0, 1.0, 0, 0)["conf_loss"])


# ------------------------------------------------------------------------------- the oracle: its gradient is its loss's
def _terms_of_s(s, pos, gamma, w_pos, w_neg):
    """The definition in float64 as a function of s (c = s + 1e-10, w = (1 - c) + 1e-10)."""
    c = s + 1e-10
    w = (1.0 - c) + 1e-10
    return FO.terms(c, w, np.ones_like(s), pos, ~pos, gamma, w_pos, w_neg)


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
@pytest.mark.parametrize("w_pos,w_neg", [(1.0, 1.0), (0.25, 0.75)])
def test_oracle_gradient_is_the_central_difference_of_its_loss(gamma, w_pos, w_neg):
    s = np.linspace(0.02, 0.98, 97)
    s = np.concatenate([s, s])
    pos = np.arange(s.size) < 97
    h = 1e-6
    _, grad = _terms_of_s(s, pos, gamma, w_pos, w_neg)
    up, _ = _terms_of_s(s + h, pos, gamma, w_pos, w_neg)
    down, _ = _terms_of_s(s - h, pos, gamma, w_pos, w_neg)
    numeric = (up - down) / (2 * h)
    # central difference in float64: truncation h^2 f'''/6 and rounding eps |f| / h are both under 1e-7 of the gradients here
    assert np.allclose(grad, numeric, rtol=1e-6, atol=1e-9)
    assert np.all(grad[pos] < 0) and np.all(grad[~pos] > 0)   # same-sign brackets: nothing cancels
    # and through the sigmoid, against the oracle's own d_conf_in
    c = make_case(4, 70, 5)
    out = FO.focal_loss(c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, gamma, w_pos, w_neg, 0, 0)
    s32, c32, w32 = FO.scw(c["z"], 1)
    _, g = FO.terms(c32.astype(np.float64), w32.astype(np.float64), np.ones(c32.shape), c["match"] >= 0, c["match"] < 0, gamma,
                    w_pos, w_neg)
    s64 = s32.astype(np.float64)
    assert np.allclose(out["d_conf_in"], g * s64 * (1 - s64), rtol=1e-6, atol=0)


@pytest.mark.parametrize("gamma", [0.0, 0.3, 0.5, 1.0, 2.0, 5.0, 10.0])
def test_everything_is_finite_at_saturation(gamma):
    for is_logit, x in ((1, [-100, -30, 30, 100]), (0, [0.0, 1.0, -0.0])):
        x = np.array([x, x], np.float32)
        match = np.stack([np.zeros(x.shape[1], np.int32), -np.ones(x.shape[1], np.int32)])
        out = FO.focal_loss(np.zeros(x.shape + (4,), np.float32), x, is_logit, np.zeros((2, 1, 4), np.float32), match, 1000.0,
                            gamma, 0.25, 0.75, 0, 0)
        assert np.isfinite(out["d_conf_in"]).all() and np.isfinite(out["conf_loss"])
        _, c, w = FO.scw(x, is_logit)
        assert c.min() >= np.float32(1e-10) and w.min() >= np.float32(1e-10)


# ------------------------------------------------------------------------------- the claim the mining ranking stands on
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0, 10.0])
@pytest.mark.parametrize("conf_is_logit", [1, 0])
def test_negative_term_is_non_decreasing_in_conf_in(gamma, conf_is_logit):
    x = np.linspace(-40, 40, 20001) if conf_is_logit else np.linspace(0, 1, 20001)
    x = np.unique(np.concatenate([x, [-100, 100] if conf_is_logit else [1e-10, 1e-7, 1 - 1e-7]]).astype(np.float32))
    _, c, w = FO.scw(x, conf_is_logit)
    term, _ = FO.terms(c.astype(np.float64), w.astype(np.float64), np.ones(x.shape), np.zeros(x.shape, bool), np.ones(x.shape, bool),
                       gamma, 1.0, 0.75)
    assert np.all(np.diff(term) >= 0) and term[-1] > term[0] >= 0


# ------------------------------------------------------------------- the bars hold for a float32 evaluation of the formulas
def _float32_restatement(c, x, is_logit, gamma, w_pos, w_neg, ulps):
    """Section 1 of the definition in float32 throughout, with s moved by `ulps` float32 steps first: what a device whose
    expf differs from numpy's by that much would compute.  The sum of the terms is taken in float64, as on the device."""
    f = np.float32
    s, _, _ = FO.scw(x, is_logit)
    for _ in range(abs(ulps)):
        s = np.nextafter(s, f(2.0) if ulps > 0 else f(-1.0))
    cc = (s + f(1e-10)).astype(f)
    ww = ((f(1.0) - cc) + f(1e-10)).astype(f)
    ds = (s * (f(1.0) - s)).astype(f) if is_logit else np.ones_like(s)
    pos = c["match"] >= 0
    term, grad = FO.terms(cc, ww, ds, pos, ~pos, gamma, w_pos, w_neg)
    assert term.dtype == f and grad.dtype == f
    return float(term.astype(np.float64).sum()), grad


@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
def test_a_float32_evaluation_stays_within_the_bars_of_the_gpu_test(B, P, G, is_logit):
    """The GPU test's bars (gradients rtol 1e-4 / atol 1e-6, confidence loss rtol 1e-5) leave room for float32 arithmetic
    and for an expf a few ulp off: shown on the GPU test's own inputs, without the GPU."""
    c = make_case(B, P, G)
    x = c["z"] if is_logit else c["x"]
    worst_grad, worst_loss = 0.0, 0.0
    for gamma in (0.5, 1.0, 2.0, 5.0):
        for w_pos, w_neg in ((1.0, 1.0), (0.25, 0.75)):
            ref = FO.focal_loss(c["dec"], x, is_logit, c["gt"], c["match"], 1000.0, gamma, w_pos, w_neg, 0, 0)
            for ulps in (-2, -1, 0, 1, 2):
                loss, grad = _float32_restatement(c, x, is_logit, gamma, w_pos, w_neg, ulps)
                ref_grad = ref["d_conf_in"].astype(np.float64)
                worst_grad = max(worst_grad, float(np.max(np.abs(grad - ref_grad) / (1e-6 + 1e-4 * np.abs(ref_grad)))))
                worst_loss = max(worst_loss, abs(loss - float(ref["conf_loss"])) / float(ref["conf_loss"]))
    print("P=%d logit=%d: worst gradient error %.3g x bar, worst confidence-loss relative error %.3g" % (P, is_logit, worst_grad, worst_loss))
    assert worst_grad <= 1.0 and worst_loss <= 1e-5


# ------------------------------------------------------------------------------------------------- MultiboxLoss keywords
def test_multibox_loss_keywords_are_validated_on_construction():
    import __graft_entry__ as g
    g.build()                                                 # the constructor asks the library for its workspace size
    from multibox_amd import loss as L, _lib
    priors = np.array([[0, 0, .5, .5], [.25, .25, 1, 1]], np.float32)
    old = L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu")
    assert old.focal is None and old.n_neg is None and old.ws.numel() == _lib.lib().mbx_loss_workspace_bytes(3)
    ml = L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", focal_gamma=2, focal_alpha=0.25)
    assert ml.focal == (2.0, 0.25, 0.75) and ml.n_neg is None
    assert ml.ws.numel() == _lib.lib().mbx_loss_focal_workspace_bytes(3, 2)
    assert L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", focal_gamma=0).focal == (0.0, 1.0, 1.0)
    mined = L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", focal_gamma=0.5, neg_per_pos=3, min_neg=1, match_iou_threshold=0.5)
    assert mined.focal == (0.5, 1.0, 1.0) and mined.n_neg.shape == (3,) and mined.n_extra.shape == (3,)
    for bad in (-0.5, 10.5, float("nan"), True, "2"):
        with pytest.raises(ValueError, match="focal_gamma"):
            L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", focal_gamma=bad)
    for bad in (0, 1, -0.25, 1.5, float("nan"), True, "0.25"):
        with pytest.raises(ValueError, match="focal_alpha"):
            L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", focal_gamma=2.0, focal_alpha=bad)
    with pytest.raises(ValueError, match="focal_alpha"):
        L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", focal_alpha=0.25)


def test_trainer_takes_the_keywords():
    import inspect
    from multibox_amd.trainer import Trainer
    p = inspect.signature(Trainer.__init__).parameters
    assert p["focal_gamma"].default is None and p["focal_alpha"].default is None


# ------------------------------------------------------------------------------------------------- ctypes table
def test_ctypes_table_declares_the_focal_entry_points():
    import ctypes as C
    from multibox_amd import _lib
    assert {"mbx_loss_focal_workspace_bytes", "mbx_loss_fwd_bwd_focal"} <= set(_lib.declared_symbols())
    res, args = _lib._SIGS["mbx_loss_fwd_bwd_focal"]
    plain = _lib._SIGS["mbx_loss_fwd_bwd"][1]
    # every argument of mbx_loss_fwd_bwd in its order, then gamma, w_pos, w_neg, neg_per_pos, min_neg, n_neg in front of
    # the workspace
    assert res is C.c_int and args == plain[:13] + [C.c_float] * 3 + [C.c_int, C.c_int, C.c_void_p] + plain[13:]
    assert _lib._SIGS["mbx_loss_focal_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int])
