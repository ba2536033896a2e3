"""IoU-aware confidence targets (mbx_loss_fwd_bwd_quality, LOSS_QUALITY_TARGET / _GAMMA / _NEG_WEIGHT), the parts that need
no GPU: the closed form of tests/quality_oracle.py against torch.autograd in float64 with q detached, anchors that do not
share its code, the config keys, the MultiboxLoss and Trainer keywords, the ctypes table against the header, the argument
checks of the entry that come before any launch, and the census of the inputs the GPU test runs on."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import focal_oracle as FO
from tests import loc_oracle as LO
from tests import quality_oracle as QO
from tests.loss_cases import ALPHA, SHAPES

T_KEY, G_KEY, W_KEY = "LOSS_QUALITY_TARGET", "LOSS_QUALITY_GAMMA", "LOSS_QUALITY_NEG_WEIGHT"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -4                                   # MBX_ERR_INVALID_ARG, MBX_ERR_WORKSPACE (include/mbx.h)


def _positives(shape, is_logit=1):
    """(q, s, c, w, ds) float64 of the positives of make_loc_case(*shape), row-major."""
    c = LO.make_loc_case(*shape)
    b, p = np.nonzero(c["match"] >= 0)
    l, g = LO.positives(c)
    s, cc, w = FO.scw(c["z"] if is_logit else c["x"], is_logit)
    s, cc, w = (a.astype(np.float64)[b, p] for a in (s, cc, w))
    return QO.iou(l, g), s, cc, w, (s * (1 - s) if is_logit else np.ones_like(s))


# ------------------------------------------------------------------------------ the closed form against autograd
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 5.0])
@pytest.mark.parametrize("mode", QO.MODES)
def test_closed_form_against_autograd_with_q_detached(mode, gamma, shape):
    q, s, c, w, _ = _positives(shape)
    L, dLds = QO.positive_terms(mode, q, s, c, w, gamma, 1.0)
    st = torch.tensor(s, requires_grad=True)
    qt = torch.tensor(q).detach()
    ct, wt = st + torch.tensor(c - s), -st + torch.tensor(w + s)     # c = s + const, w = -s + const: the float32 values
    t = qt * torch.log(ct) + (1 - qt) * torch.log(wt)
    M = qt if mode == "varifocal" else (torch.ones_like(st) if gamma == 0 else torch.abs(qt - st) ** gamma)
    Lt = -(M * t)
    grad, = torch.autograd.grad(Lt.sum(), st)
    assert np.isfinite(L).all() and np.isfinite(dLds).all()
    assert np.allclose(L, Lt.detach().numpy(), rtol=1e-10, atol=0)
    assert np.allclose(dLds, grad.numpy(), rtol=1e-10, atol=0)


# ----------------------------------------------------------------------------------------------------- anchors
def test_varifocal_with_q_zero_gives_exactly_nothing():
    s, c, w = (a.astype(np.float64) for a in FO.scw(np.array([0.0, 0.3, 1.0, 0.999], np.float32), 0))     # c, w >= 1e-10
    for gamma in (0.0, 2.0):
        L, d = QO.positive_terms("varifocal", np.zeros(4), s, c, w, gamma)
        assert np.all(L == 0) and np.all(d == 0)


def test_qfl_gamma_zero_q_one_is_the_plain_positive():
    s, c, w = (a.astype(np.float64) for a in FO.scw(np.array([0.1, 0.5, 0.9], np.float32), 0))
    L, d = QO.positive_terms("qfl", np.ones(3), s, c, w, 0.0)
    assert np.array_equal(L, -np.log(c)) and np.array_equal(d, -1.0 / c)
    ds = s * (1 - s)
    assert np.allclose(d * ds, -ds / c, rtol=0, atol=0)


def test_qfl_at_q_equal_s_passes_nothing_and_by_hand():
    s, c, w = (a.astype(np.float64) for a in FO.scw(np.array([0.0, 0.25], np.float32), 0))
    for gamma in (1.0, 2.0, 5.0):
        L, d = QO.positive_terms("qfl", s.copy(), s, c, w, gamma)
        assert np.all(L == 0) and np.all(d == 0)
    # q = 0.75, s = 0.25, gamma = 2: M = 1/4, dM = -1, t = .75 log .25 + .25 log .75, dt = 3 - 1/3 (the epsilons: 1e-9)
    L, d = QO.positive_terms("qfl", [0.75], [0.25], [0.25], [0.75], 2.0)
    t = 0.75 * np.log(0.25) + 0.25 * np.log(0.75)
    assert np.isclose(L[0], -0.25 * t, rtol=1e-14) and np.isclose(d[0], -(-1.0 * t + 0.25 * (3 - 1 / 3)), rtol=1e-14)
    L, d = QO.positive_terms("varifocal", [0.75], [0.25], [0.25], [0.75], 2.0, w_pos=2.0)
    assert np.isclose(L[0], -2 * 0.75 * t, rtol=1e-14) and np.isclose(d[0], -2 * 0.75 * (3 - 1 / 3), rtol=1e-14)


@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_the_negatives_and_the_location_side_are_the_other_oracles(neg_per_pos):
    c = LO.make_loc_case(4, 70, 5)
    ref = QO.quality_loss("qfl", "giou", c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA, 2.0, 1.0, 0.75, neg_per_pos)
    focal = LO.loc_loss("giou", c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA, gamma=2.0, w_pos=0.25, w_neg=0.75,
                        neg_per_pos=neg_per_pos)
    neg = c["match"] < 0
    assert np.array_equal(ref["mask"], focal["mask"]) and np.array_equal(ref["n_neg"], focal["n_neg"])
    assert np.array_equal(ref["d_conf_in"][neg].astype(np.float32), focal["d_conf_in"][neg])
    assert ref["loc_loss"] == focal["loc_loss"] and np.array_equal(ref["dl"], focal["dl"])
    # a negative's term is focal_oracle's: the focal total less its positives' terms
    s, cc, w = (a.astype(np.float64) for a in FO.scw(c["z"], 1))
    term, _ = FO.terms(cc, w, s * (1 - s), ~neg, np.zeros_like(neg), 2.0, 0.25, 0.75,
                       np.log(cc.astype(np.float32)).astype(np.float64), np.log(w.astype(np.float32)).astype(np.float64))
    assert np.isclose(ref["neg_loss"], float(focal["conf_loss"]) - term.sum(), rtol=1e-6)
    assert np.isclose(ref["conf_loss"], ref["neg_loss"] + ref["L"].sum(), rtol=1e-15)
    assert np.array_equal(ref["q_stats"][:, 1], (~neg).sum(1)) and np.isclose(ref["q_stats"][:, 0].sum(), ref["q"].sum(), rtol=1e-14)


# ----------------------------------------------------------------------------- the inputs of the GPU test
@pytest.mark.parametrize("shape", SHAPES)
def test_the_gpu_tests_inputs_hold_disjoint_and_overlapping_positives_away_from_the_kink(shape):
    for is_logit in (1, 0):
        q, s, _, _, _ = _positives(shape, is_logit)
        assert 1 <= int((q == 0).sum()) <= 6 and int(((q > 0.3) & (q < 0.95)).sum()) >= 8
        assert np.abs(q - s).min() >= 1e-3
    c = LO.make_loc_case(*shape)
    assert np.abs(c["z"][c["match"] >= 0]).max() <= 8.5       # the positives' logits: s is no ulp-sensitive input there


def test_two_ulps_of_s_stay_far_inside_the_bars():
    """The device's expf differs from numpy's by an ulp or two of s: what that moves, against the GPU test's bars (gradients
    rtol 1e-4 / atol 1e-6, loss rtol 1e-5)."""
    q, s, _, _, ds = _positives((2, 3199, 100))
    for mode in QO.MODES:
        for gamma in (0.0, 1.0, 2.0, 5.0):
            def at(s32):
                s64 = s32.astype(np.float64)
                c = (s32 + np.float32(1e-10)).astype(np.float64)
                w = ((np.float32(1) - (s32 + np.float32(1e-10))) + np.float32(1e-10)).astype(np.float64)
                L, d = QO.positive_terms(mode, q, s64, c, w, gamma)
                return L, d * ds
            s32 = s.astype(np.float32)
            moved = np.nextafter(np.nextafter(s32, np.float32(2)), np.float32(2))
            (L0, g0), (L1, g1) = at(s32), at(moved)
            worst = float(np.max(np.abs(g1 - g0) / (1e-6 + 1e-4 * np.abs(g0))))
            assert worst <= 0.12, (mode, gamma, worst)
            assert abs(L1.sum() - L0.sum()) <= 2e-5 * abs(L0.sum())


# ------------------------------------------------------------------------------------------------- config keys
@pytest.mark.parametrize("cfg,want", [
    ({}, None), ({T_KEY: None}, None), ({T_KEY: None, G_KEY: None, W_KEY: None}, None),
    ({T_KEY: "qfl"}, ("qfl", 2.0, 1.0)), ({T_KEY: "varifocal"}, ("varifocal", 2.0, 0.75)),
    ({T_KEY: "qfl", G_KEY: 0}, ("qfl", 0.0, 1.0)), ({T_KEY: "qfl", G_KEY: 1}, ("qfl", 1.0, 1.0)),
    ({T_KEY: "qfl", G_KEY: 10, W_KEY: 0.5}, ("qfl", 10.0, 0.5)), ({T_KEY: "varifocal", G_KEY: 0.5}, ("varifocal", 0.5, 0.75)),
    ({T_KEY: "varifocal", G_KEY: None, W_KEY: 2}, ("varifocal", 2.0, 2.0)),
    ({T_KEY: "qfl", "LOSS_LOC_TYPE": "giou", "LOSS_NEG_PER_POS": 3, "LOSS_MATCH_ATSS_TOPK": 9}, ("qfl", 2.0, 1.0)),
])
def test_quality_loss_accepts(cfg, want):
    from multibox_amd.config import Cfg, quality_loss, with_defaults
    for c in (Cfg(cfg), with_defaults(Cfg(cfg))):             # the defaults switch nothing on
        got = quality_loss(c)
        if want is None:
            assert got is None
        else:
            assert got == dict(quality_target=want[0], quality_gamma=want[1], quality_neg_weight=want[2])
            assert type(got["quality_gamma"]) is float and type(got["quality_neg_weight"]) is float


@pytest.mark.parametrize("cfg,key", [({T_KEY: v}, T_KEY) for v in ("QFL", "vfl", "", 0, 1, 2.0, True, False, ["qfl"])]
                         + [({T_KEY: t, G_KEY: v}, G_KEY) for t in QO.MODES
                            for v in (-0.5, 10.5, True, False, "2", [2], float("nan"), float("inf"), -float("inf"))]
                         + [({T_KEY: "qfl", G_KEY: v}, G_KEY) for v in (0.5, 0.999, 1e-3, 1e-60)]
                         + [({T_KEY: t, W_KEY: v}, W_KEY) for t in QO.MODES
                            for v in (0, 0.0, -0.75, True, False, "1", [1], float("nan"), float("inf"), 1e-60, 1e60)]
                         + [({G_KEY: 2}, G_KEY), ({W_KEY: 1.0}, W_KEY), ({T_KEY: None, G_KEY: 2}, G_KEY),
                            ({T_KEY: None, W_KEY: 0.75}, W_KEY)])
def test_quality_loss_rejects(cfg, key):
    from multibox_amd.config import Cfg, quality_loss
    with pytest.raises(ValueError, match=key):
        quality_loss(Cfg(cfg))


@pytest.mark.parametrize("other", [{"LOSS_FOCAL_GAMMA": 2}, {"LOSS_FOCAL_ALPHA": 0.25}, {"LOSS_FOCAL_GAMMA": 0, "LOSS_FOCAL_ALPHA": 0.25}])
def test_quality_loss_beside_the_focal_keys_names_both(other):
    from multibox_amd.config import Cfg, quality_loss
    with pytest.raises(ValueError) as e:
        quality_loss(Cfg(dict(other, **{T_KEY: "varifocal"})))
    assert T_KEY in str(e.value) and sorted(other)[-1] in str(e.value)
    assert quality_loss(Cfg(other)) is None                   # the focal keys alone are the focal loss's business


def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch):
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\n%s: qfl\n%s: 0.5\n" % (T_KEY, G_KEY))

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match=G_KEY):
        train.main()


# ------------------------------------------------------------------------- MultiboxLoss / Trainer keywords
def test_multibox_loss_keywords_select_the_entry():
    import __graft_entry__ as g
    g.build()                                                 # the constructor asks the library for its workspace size
    from multibox_amd import loss as L, _lib
    l = _lib.lib()
    priors = np.array([[0, 0, .5, .5], [.25, .25, 1, 1]], np.float32)
    new = lambda **kw: L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", **kw)
    # without the switch: the entry, its arguments and its workspace are what they were
    for kw, entry, n_args, ws in ((dict(), "mbx_loss_fwd_bwd", 0, l.mbx_loss_workspace_bytes(3)),
                                  (dict(neg_per_pos=3), "mbx_loss_fwd_bwd_mined", 3, l.mbx_loss_mined_workspace_bytes(3, 2)),
                                  (dict(focal_gamma=2.0), "mbx_loss_fwd_bwd_focal", 6, l.mbx_loss_focal_workspace_bytes(3, 2)),
                                  (dict(loc_loss="giou"), "mbx_loss_fwd_bwd_loc", 8, l.mbx_loss_loc_workspace_bytes(3, 2))):
        for m in (new(**kw), new(quality_target=None, quality_gamma=None, quality_neg_weight=None, **kw)):
            assert m.quality is None and m.q_stats is None
            assert m.entry == entry and len(m.entry_args) == n_args and m.ws.numel() == ws
    assert new(focal_gamma=2.0).entry_args == (2.0, 1.0, 1.0, 0, 0, None)
    assert new(loc_loss="giou").entry_args == (2, 0.0, 0.0, 1.0, 1.0, 0, 0, None)
    # with it: the one entry -- (loc_type, loc_beta), (quality, gamma, w_pos = 1, w_neg), the mining arguments, q_stats
    assert L.QUALITY_TARGETS == QO.MODES
    m = new(quality_target="qfl")
    assert m.entry == "mbx_loss_fwd_bwd_quality" and m.ws.numel() == l.mbx_loss_quality_workspace_bytes(3, 2)
    assert m.q_stats.shape == (3, 2) and m.q_stats.dtype == torch.float64 and m.n_neg is None
    assert m.entry_args == (0, 0.0, 1, 2.0, 1.0, 1.0, 0, 0, None, m.q_stats.data_ptr())
    m = new(quality_target="varifocal")
    assert m.entry_args == (0, 0.0, 2, 2.0, 1.0, 0.75, 0, 0, None, m.q_stats.data_ptr())
    m = new(quality_target="varifocal", quality_gamma=1.5, quality_neg_weight=0.5, loc_loss="smooth_l1", loc_beta=0.5,
            neg_per_pos=3, min_neg=1, match_iou_threshold=0.5)
    assert m.entry == "mbx_loss_fwd_bwd_quality" and m.n_extra.shape == (3,)
    assert m.entry_args == (1, 0.5, 2, 1.5, 1.0, 0.5, 3, 1, m.n_neg.data_ptr(), m.q_stats.data_ptr())
    assert len(m.entry_args) + 13 + 3 == len(_lib._SIGS["mbx_loss_fwd_bwd_quality"][1])
    assert l.mbx_loss_quality_workspace_bytes(3, 2) == l.mbx_loss_workspace_bytes(3)
    assert new(quality_target="varifocal", quality_gamma=0.5).quality == (2, 0.5, 1.0, 0.75)     # below 1 is QFL's limit only
    for bad in ("QFL", "vfl", 1, True, ["qfl"]):
        with pytest.raises(ValueError, match="quality_target"):
            new(quality_target=bad)
    for bad in (-0.5, 10.5, float("nan"), float("inf"), True, "2", 0.5, 0.999):
        with pytest.raises(ValueError, match="quality_gamma"):
            new(quality_target="qfl", quality_gamma=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), 1e-60, True, "1"):
        with pytest.raises(ValueError, match="quality_neg_weight"):
            new(quality_target="varifocal", quality_neg_weight=bad)
    with pytest.raises(ValueError, match="quality_gamma"):
        new(quality_gamma=2.0)
    with pytest.raises(ValueError, match="quality_neg_weight"):
        new(quality_neg_weight=1.0)
    for kw in (dict(focal_gamma=2.0), dict(focal_gamma=0.0, focal_alpha=0.25)):
        with pytest.raises(ValueError) as e:
            new(quality_target="qfl", **kw)
        assert "quality_target" in str(e.value) and "focal_gamma" in str(e.value)


def test_trainer_takes_the_keywords_and_reports_the_mean_iou():
    from multibox_amd.trainer import Trainer
    p = inspect.signature(Trainer.__init__).parameters
    assert all(p[k].default is None for k in ("quality_target", "quality_gamma", "quality_neg_weight"))

    class Loss:
        q_stats = None
    tr = Trainer.__new__(Trainer)
    tr.loss = Loss()
    assert tr.mean_positive_iou() is None
    tr.loss.q_stats = torch.tensor([[0.0, 0.0], [1.5, 3.0], [0.5, 1.0]], dtype=torch.float64)
    assert tr.mean_positive_iou() == 0.5
    tr.loss.q_stats = torch.zeros((2, 2), dtype=torch.float64)
    assert tr.mean_positive_iou() == 0.0


# ------------------------------------------------------------------------------- ctypes table and header
def test_ctypes_table_and_header_agree_on_the_quality_entry():
    from multibox_amd import _lib
    assert {"mbx_loss_quality_workspace_bytes", "mbx_loss_fwd_bwd_quality"} <= set(_lib.declared_symbols())
    res, args = _lib._SIGS["mbx_loss_fwd_bwd_quality"]
    loc = _lib._SIGS["mbx_loss_fwd_bwd_loc"][1]
    # every argument of mbx_loss_fwd_bwd_loc in its order, with quality in front of gamma and q_stats behind n_neg
    assert res is C.c_int and args == loc[:15] + [C.c_int] + loc[15:21] + [C.c_void_p] + loc[21:]
    assert _lib._SIGS["mbx_loss_quality_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int])
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbx.h")).read(), flags=re.S)
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p,
             "double*": C.c_void_p, "void*": C.c_void_p, "mbx_stream_t": C.c_void_p, "int": C.c_int, "float": C.c_float,
             "size_t": C.c_size_t}
    for name in ("mbx_loss_fwd_bwd_quality", "mbx_loss_quality_workspace_bytes"):
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr).groups()
        params = [" ".join(p.split()) for p in params.split(",")]
        assert [ctype[p.rsplit(" ", 1)[0]] for p in params] == _lib._SIGS[name][1], name
        assert ctype[ret] is _lib._SIGS[name][0]
        if name == "mbx_loss_fwd_bwd_quality":
            names = [p.rsplit(" ", 1)[1] for p in params]
            assert names[13:19] == ["loc_type", "loc_beta", "quality", "gamma", "w_pos", "w_neg"] and names[21:23] == ["n_neg", "q_stats"]
    enum = re.search(r"enum\s*\{([^}]*MBX_QUALITY_NONE[^}]*)\}", hdr).group(1)
    values = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(","))}
    assert values == {"MBX_QUALITY_NONE": 0, "MBX_QUALITY_QFL": 1, "MBX_QUALITY_VFL": 2}


# ------------------------------------------------------------------ the checks that come before any launch
def test_the_entry_refuses_bad_arguments_before_any_launch():
    """Pointers here are made-up addresses: every call must be refused before anything is launched or read."""
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    l = _lib.lib()
    A = 0x10000
    assert l.mbx_loss_quality_workspace_bytes(4, 70) == l.mbx_loss_loc_workspace_bytes(4, 70) == 64
    order = ("dec", "z", "is_logit", "gt", "match", "alpha", "grad_scale", "B", "P", "G", "loss2", "dl", "dz", "loc_type", "beta",
             "quality", "gamma", "w_pos", "w_neg", "neg_per_pos", "min_neg", "n_neg", "q_stats", "ws", "ws_bytes", "stream")
    good = dict(dec=A, z=A, is_logit=1, gt=A, match=A, alpha=1000.0, grad_scale=1.0, B=4, P=70, G=5, loss2=A, dl=A, dz=A,
                loc_type=2, beta=0.0, quality=1, gamma=2.0, w_pos=1.0, w_neg=1.0, neg_per_pos=0, min_neg=0, n_neg=A,
                q_stats=A, ws=A, ws_bytes=64, stream=None)
    go = lambda **kw: l.mbx_loss_fwd_bwd_quality(*[dict(good, **kw)[k] for k in order])
    for kw in (dict(quality=-1), dict(quality=3), dict(quality=0), dict(quality=0, q_stats=A, ws_bytes=0),
               dict(gamma=0.5), dict(gamma=0.999), dict(gamma=1e-3), dict(gamma=0.5, ws_bytes=0),
               dict(gamma=-0.5), dict(gamma=10.5), dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(quality=2, gamma=float("nan")), dict(quality=2, gamma=-1.0),
               dict(w_pos=-1.0), dict(w_neg=-1.0), dict(w_pos=float("inf")), dict(w_neg=float("nan")),
               dict(loc_type=-1), dict(loc_type=5), dict(loc_type=1, beta=0.0), dict(loc_type=1, beta=float("nan")),
               dict(neg_per_pos=-1), dict(neg_per_pos=3, min_neg=-1), dict(neg_per_pos=0, min_neg=1),
               dict(dec=None), dict(z=None), dict(gt=None), dict(match=None), dict(loss2=None), dict(B=0), dict(B=-1), dict(P=0),
               dict(G=0), dict(quality=5, ws_bytes=0), dict(loc_type=5, ws=None)):
        assert go(**kw) == INVALID, kw
    for kw in (dict(ws=None), dict(ws_bytes=63), dict(ws_bytes=0, quality=2), dict(ws_bytes=63, neg_per_pos=3),
               dict(ws_bytes=63, quality=0, q_stats=None), dict(ws_bytes=63, quality=2, gamma=0.5),
               dict(ws_bytes=63, dl=None, dz=None, n_neg=None, q_stats=None)):
        assert go(**kw) == WORKSPACE, kw
