"""The choice of location term (mbx_loss_fwd_bwd_loc, LOSS_LOC_TYPE / LOSS_LOC_BETA), the parts that need no GPU: the config
keys, the MultiboxLoss and Trainer keywords, the ctypes table against the header, the inputs of the GPU test (how many
positives are inverted, disjoint, near a kink) and the float64 autograd restatement the GPU tests compare against
(tests/loc_oracle.py), anchored to things that do not share its code: ref_numpy's L2, torch's smooth_l1_loss, identities
between the IoU types, and values worked by hand."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import focal_oracle as FO
from tests import loc_oracle as LO
from tests.loss_cases import ALPHA, SHAPES, make_case

T_KEY, B_KEY = "LOSS_LOC_TYPE", "LOSS_LOC_BETA"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- config keys
@pytest.mark.parametrize("cfg,want", [
    ({}, None),
    ({T_KEY: None}, None),
    ({T_KEY: None, B_KEY: None}, None),
    ({T_KEY: "l2"}, ("l2", None)),
    ({T_KEY: "smooth_l1"}, ("smooth_l1", 0.1)),
    ({T_KEY: "smooth_l1", B_KEY: None}, ("smooth_l1", 0.1)),
    ({T_KEY: "smooth_l1", B_KEY: 1}, ("smooth_l1", 1.0)),
    ({T_KEY: "smooth_l1", B_KEY: 0.02}, ("smooth_l1", 0.02)),
    ({T_KEY: "giou"}, ("giou", None)),
    ({T_KEY: "diou", B_KEY: None}, ("diou", None)),
    ({T_KEY: "ciou"}, ("ciou", None)),
])
def test_loc_loss_accepts(cfg, want):
    from multibox_amd.config import Cfg, loc_loss, with_defaults
    assert loc_loss(Cfg(cfg)) == want
    got = loc_loss(with_defaults(Cfg(cfg)))                   # the defaults switch nothing on
    assert got == want and (got is None or type(got[1]) in (float, type(None)))


@pytest.mark.parametrize("cfg,key", [({T_KEY: v}, T_KEY) for v in ("L2", "iou", "smooth-l1", "", 0, 2, 1.0, True, False, ["giou"])]
                         + [({T_KEY: "smooth_l1", B_KEY: v}, B_KEY) for v in (0, 0.0, -0.1, True, False, "0.1", [0.1], float("nan"),
                                                                              float("inf"), -float("inf"), 1e-60, 1e60)]
                         + [({T_KEY: t, B_KEY: 0.1}, B_KEY) for t in ("l2", "giou", "diou", "ciou")]
                         + [({B_KEY: 0.1}, B_KEY), ({T_KEY: None, B_KEY: 0.1}, B_KEY)])
def test_loc_loss_rejects(cfg, key):
    from multibox_amd.config import Cfg, loc_loss
    with pytest.raises(ValueError, match=key):
        loc_loss(Cfg(cfg))


def test_the_loc_keys_compose_with_mining_focal_and_threshold_matching():
    from multibox_amd.config import Cfg, focal_loss, loc_loss, match_iou_threshold, negative_mining
    cfg = Cfg({T_KEY: "smooth_l1", B_KEY: 0.05, "LOSS_FOCAL_GAMMA": 2, "LOSS_FOCAL_ALPHA": 0.25, "LOSS_NEG_PER_POS": 3,
               "LOSS_MATCH_IOU_THRESHOLD": 0.4})
    assert loc_loss(cfg) == ("smooth_l1", 0.05) and focal_loss(cfg) == (2.0, 0.25) and negative_mining(cfg) == (3, 0)
    assert match_iou_threshold(cfg) == 0.4
    assert loc_loss(Cfg({"LOSS_FOCAL_GAMMA": 2, "LOSS_NEG_PER_POS": 3, "LOSS_MATCH_IOU_THRESHOLD": 0.4})) is None
    only = Cfg({T_KEY: "ciou"})
    assert focal_loss(only) is None and negative_mining(only) is None and match_iou_threshold(only) is None
    from multibox_amd.config import DEFAULTS
    assert DEFAULTS["LOCATION_LOSS_ALPHA"] == 1000.0          # sized for L2; the IoU types' users set their own


def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch):
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\n%s: giou\n%s: 0.1\n" % (T_KEY, B_KEY))

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match=B_KEY):
        train.main()


def test_train_log_gains_loc_loss_and_beta_for_smooth_l1_only():
    import train
    from multibox_amd.config import Cfg, loc_loss
    fields = lambda cfg: train.loc_log_fields(loc_loss(Cfg(cfg)))
    assert fields({}) == {} and fields({T_KEY: None}) == {}
    assert fields({T_KEY: "giou"}) == {"loc_loss": "giou"} and fields({T_KEY: "l2"}) == {"loc_loss": "l2"}
    assert fields({T_KEY: "smooth_l1"}) == {"loc_loss": "smooth_l1", "loc_beta": 0.1}
    assert fields({T_KEY: "smooth_l1", B_KEY: 0.5}) == {"loc_loss": "smooth_l1", "loc_beta": 0.5}


# ------------------------------------------------------------------------------------- MultiboxLoss / Trainer keywords
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
                                  (dict(focal_gamma=2.0), "mbx_loss_fwd_bwd_focal", 6, l.mbx_loss_focal_workspace_bytes(3, 2))):
        for m in (new(**kw), new(loc_loss=None, loc_beta=None, **kw)):
            assert m.loc is None and m.entry == entry and len(m.entry_args) == n_args and m.ws.numel() == ws
    assert new().entry_args == () and new(focal_gamma=2.0).entry_args == (2.0, 1.0, 1.0, 0, 0, None)
    # with it: the one entry, (loc_type, loc_beta) in front of the focal arguments, (0, 1, 1) when the focal loss is off
    assert L.LOC_TYPES == LO.TYPES
    for t, name in enumerate(L.LOC_TYPES):
        m = new(loc_loss=name)
        assert m.entry == "mbx_loss_fwd_bwd_loc" and m.ws.numel() == l.mbx_loss_loc_workspace_bytes(3, 2)
        assert m.entry_args == (t, 0.1 if name == "smooth_l1" else 0.0, 0.0, 1.0, 1.0, 0, 0, None) and m.n_neg is None
    m = new(loc_loss="smooth_l1", loc_beta=0.5, focal_gamma=2, focal_alpha=0.25, neg_per_pos=3, min_neg=1, match_iou_threshold=0.5)
    assert m.entry == "mbx_loss_fwd_bwd_loc" and m.n_extra.shape == (3,)
    assert m.entry_args == (1, 0.5, 2.0, 0.25, 0.75, 3, 1, m.n_neg.data_ptr())
    assert l.mbx_loss_loc_workspace_bytes(3, 2) == l.mbx_loss_workspace_bytes(3)
    for bad in ("iou", "L2", 2, True, ["giou"]):
        with pytest.raises(ValueError, match="loc_loss"):
            new(loc_loss=bad)
    for bad in (0, 0.0, -0.1, float("nan"), float("inf"), 1e-60, True, "0.1"):
        with pytest.raises(ValueError, match="loc_beta"):
            new(loc_loss="smooth_l1", loc_beta=bad)
    for kw in (dict(loc_beta=0.1), dict(loc_loss="giou", loc_beta=0.1), dict(loc_loss="l2", loc_beta=0.1)):
        with pytest.raises(ValueError, match="loc_beta"):
            new(**kw)


def test_trainer_takes_the_keywords():
    import inspect
    from multibox_amd.trainer import Trainer
    p = inspect.signature(Trainer.__init__).parameters
    assert p["loc_loss"].default is None and p["loc_beta"].default is None


# ------------------------------------------------------------------------------------------- ctypes table and header
def test_ctypes_table_and_header_agree_on_the_loc_entry():
    import ctypes as C
    from multibox_amd import _lib
    assert {"mbx_loss_loc_workspace_bytes", "mbx_loss_fwd_bwd_loc"} <= set(_lib.declared_symbols())
    res, args = _lib._SIGS["mbx_loss_fwd_bwd_loc"]
    focal = _lib._SIGS["mbx_loss_fwd_bwd_focal"][1]
    # every argument of mbx_loss_fwd_bwd_focal in its order, with loc_type and loc_beta in front of gamma
    assert res is C.c_int and args == focal[:13] + [C.c_int, C.c_float] + focal[13:]
    assert _lib._SIGS["mbx_loss_loc_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int])
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbx.h")).read(), flags=re.S)
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p,
             "void*": C.c_void_p, "mbx_stream_t": C.c_void_p, "int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}
    for name in ("mbx_loss_fwd_bwd_loc", "mbx_loss_fwd_bwd_focal", "mbx_loss_loc_workspace_bytes"):
        ret, params = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr).groups()
        params = [" ".join(p.split()) for p in params.split(",")]
        names = [p.rsplit(" ", 1)[1] for p in params]
        assert [ctype[p.rsplit(" ", 1)[0]] for p in params] == _lib._SIGS[name][1], name
        assert ctype[ret] is _lib._SIGS[name][0]
        if name == "mbx_loss_fwd_bwd_loc":
            assert names[13:16] == ["loc_type", "loc_beta", "gamma"]
    enum = re.search(r"enum\s*\{([^}]*MBX_LOC_L2[^}]*)\}", hdr).group(1)
    values = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(","))}
    assert values == {"MBX_LOC_" + t.upper(): i for i, t in enumerate(LO.TYPES)}


# ---------------------------------------------------------------------------------------- the inputs of the GPU test
@pytest.mark.parametrize("shape,positives,inverted,disjoint", [((3, 13, 13), 22, 5, 2), ((4, 70, 5), 11, 0, 1),
                                                               ((4, 646, 13), 38, 6, 4), ((2, 3199, 100), 100, 18, 6)])
def test_the_gpu_tests_inputs_hold_every_kind_of_pair_and_no_kink(shape, positives, inverted, disjoint):
    assert shape in SHAPES
    c = LO.make_loc_case(*shape)
    plain = make_case(*shape)
    for k in ("match", "z", "x"):
        assert np.array_equal(c[k], plain[k])
    assert np.all(c["gt"][..., 2:] > c["gt"][..., :2]) and c["dec"].dtype == np.float32 and c["gt"].dtype == np.float32
    l, g = LO.positives(c)
    inv, dis, over = LO.census(l, g)
    assert (len(l), inv, dis) == (positives, inverted, disjoint) and over == positives - disjoint
    if positives >= 20:
        assert inv >= 1 and dis >= 1 and over >= 1
    # no positive within 1e-5 of a kink of any type: no element has to be left out of the gradient comparison
    assert int((LO.kink_distances(l, g, LO.BETA) < 1e-5).sum()) == 0
    r = np.abs(l - g)
    assert (r < LO.BETA).any() and (r > LO.BETA).any()        # both branches of smooth-L1 are taken


# --------------------------------------------------------------------------------------------------- the oracle: anchors
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_l2_is_the_focal_oracles_location_side(B, P, G):
    c = LO.make_loc_case(B, P, G)
    out = LO.loc_loss("l2", c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA)
    ref = FO.focal_loss(c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA, 0.0, 1.0, 1.0, 0, 0)
    # ref_numpy sums in float32 steps of its own; the float64 sum agrees to float32 rounding
    assert np.isclose(out["loc_loss"], float(ref["loc_loss"]), rtol=1e-6)
    assert np.array_equal(out["dl"].astype(np.float32), ref["d_locs"])
    assert out["conf_loss"].tobytes() == ref["conf_loss"].tobytes() and np.array_equal(out["d_conf_in"], ref["d_conf_in"])
    assert not out["dl"][c["match"] < 0].any()


@pytest.mark.parametrize("beta", [0.1, 0.02, 1.0])
def test_smooth_l1_is_torchs(beta):
    c = LO.make_loc_case(4, 646, 13)
    l, g = LO.positives(c)
    L, grad = LO.box_loss_and_grad("smooth_l1", l, g, beta)
    lt = torch.tensor(l, requires_grad=True)
    ref = torch.nn.functional.smooth_l1_loss(lt, torch.tensor(g), beta=beta, reduction="sum")
    ref_grad, = torch.autograd.grad(ref, lt)
    assert np.isclose(L.sum(), float(ref.detach()), rtol=1e-13) and np.allclose(grad, ref_grad.numpy(), rtol=1e-13, atol=0)
    # |d| == beta exactly takes the linear branch: value beta / 2 either way, slope 1 -- and by hand
    L, grad = LO.box_loss_and_grad("smooth_l1", [[beta, 0.0, -beta, 0.0]], [[0.0, 0.0, 0.0, 0.0]], beta)
    assert np.isclose(L[0], beta) and grad.tolist() == [[1.0, 0.0, -1.0, 0.0]]
    L, grad = LO.box_loss_and_grad("smooth_l1", [[0.05, 0.1, 0.2, -0.3]], [[0.0, 0.0, 0.0, 0.0]], 0.1)
    assert np.isclose(L[0], 0.0125 + 0.05 + 0.15 + 0.25, rtol=1e-14) and np.allclose(grad, [[0.5, 1.0, 1.0, -1.0]], rtol=1e-14)


def test_ciou_is_diou_when_the_aspect_ratios_are_equal():
    rng = np.random.RandomState(3)
    g = np.concatenate([rng.uniform(0, .5, (40, 2)), rng.uniform(.5, 1, (40, 2))], 1)
    scale, shift = rng.uniform(.3, 2, (40, 1)), rng.uniform(-.2, .2, (40, 2))
    wh = (g[:, 2:] - g[:, :2]) * scale                        # the same w / h as the gt box, another size and place
    l = np.concatenate([g[:, :2] + shift, g[:, :2] + shift + wh], 1)
    Lc, gc = LO.box_loss_and_grad("ciou", l, g)
    Ld, gd = LO.box_loss_and_grad("diou", l, g)
    # v = (4 / pi^2) delta^2 with delta at rounding (1e-16): a v = v^2 / (...) is far under the 1e-12 allowed here
    assert np.allclose(Lc, Ld, rtol=0, atol=1e-12) and np.allclose(gc, gd, rtol=0, atol=1e-12)
    l[:, 2] += 0.3                                            # another aspect ratio: the term is there
    assert np.all(LO.box_loss_and_grad("ciou", l, g)[0] > LO.box_loss_and_grad("diou", l, g)[0])


def test_giou_is_one_minus_iou_when_the_enclosing_box_is_the_union():
    g = np.array([[.1, .2, .5, .6], [.1, .2, .5, .6], [.3, .3, .4, .9]])
    l = g.copy()
    l[0, 2], l[1, 0], l[2, 3] = .9, -.2, .5                   # the same box stretched or shrunk along one axis
    L, _ = LO.box_loss_and_grad("giou", l, g)
    q = LO.iou_parts(torch.tensor(l), torch.tensor(g))
    assert np.allclose(q["cw"] * q["ch"], q["union"], rtol=1e-14)
    assert np.allclose(L, 1 - q["iou"].numpy(), rtol=0, atol=1e-15)


@pytest.mark.parametrize("loc_type", ["giou", "diou", "ciou"])
def test_swapping_x1_and_x2_keeps_the_term_and_swaps_the_gradients(loc_type):
    c = LO.make_loc_case(2, 3199, 100)
    l, g = LO.positives(c)
    L, grad = LO.box_loss_and_grad(loc_type, l, g)
    L2, grad2 = LO.box_loss_and_grad(loc_type, l[:, [2, 1, 0, 3]], g)
    assert np.array_equal(L, L2) and np.array_equal(grad[:, [2, 1, 0, 3]], grad2)
    L3, grad3 = LO.box_loss_and_grad(loc_type, l[:, [0, 3, 2, 1]], g)
    assert np.array_equal(L, L3) and np.array_equal(grad[:, [0, 3, 2, 1]], grad3)


def test_values_by_hand():
    e = LO.EPS
    unit = [0.0, 0.0, 1.0, 1.0]
    # equal boxes: IoU = 1 / (1 + eps), nothing else
    for t in ("giou", "diou", "ciou"):
        L, grad = LO.box_loss_and_grad(t, [unit], [unit])
        assert np.isclose(L[0], 1 - 1 / (1 + e), rtol=1e-8, atol=1e-20) and np.isfinite(grad).all()
    # nested, concentric, same aspect ratio: I = 1/4, U = 1, the enclosing box is the gt box
    inner = [0.25, 0.25, 0.75, 0.75]
    for t in ("giou", "diou", "ciou"):
        L, grad = LO.box_loss_and_grad(t, [inner], [unit])
        assert np.isclose(L[0], 1 - 0.25 / (1 + e), rtol=1e-14)
        # growing the inner box raises the IoU: dI = h = 1/2 per corner, dU = 0 while it stays inside
        assert np.allclose(grad, np.array([[0.5, 0.5, -0.5, -0.5]]) / (1 + e), rtol=1e-12)
    # disjoint, side by side: I = 0, U = 2, enclosing 3 x 1, centres 2 apart
    away = [2.0, 0.0, 3.0, 1.0]
    L, grad = LO.box_loss_and_grad("giou", [away], [unit])
    assert np.isclose(L[0], 1 + 1 / (3 + e), rtol=1e-14)
    # t = (C - U) / (C + eps), C = x2 (y2 - y1) and U = 1 + (x2 - x1)(y2 - y1) here: by hand at the point
    C, U = 3.0, 2.0
    dC, dU = np.array([0.0, -3.0, 1.0, 3.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    assert np.allclose(grad[0], (dC - dU) / (C + e) - (C - U) * dC / (C + e) ** 2, rtol=1e-12)
    L, grad = LO.box_loss_and_grad("diou", [away], [unit])
    assert np.isclose(L[0], 1 + 4 / (10 + e), rtol=1e-14)
    L, _ = LO.box_loss_and_grad("ciou", [away], [unit])
    assert np.isclose(L[0], 1 + 4 / (10 + e), rtol=1e-14)      # both square: v = 0
    # ciou with different aspect ratios: v and a by hand
    wide = [0.0, 0.0, 2.0, 1.0]
    L, _ = LO.box_loss_and_grad("ciou", [wide], [unit])
    iou = 1 / (2 + e)
    v = 4 / math.pi ** 2 * (math.atan2(1, 1) - math.atan2(2, 1)) ** 2
    assert np.isclose(L[0], 1 - iou + 0.25 / (5 + e) + v * v / (1 - iou + v + e), rtol=1e-14)


@pytest.mark.parametrize("loc_type", LO.TYPES)
def test_degenerate_boxes_give_finite_terms_and_gradients(loc_type):
    from tests.test_gpu_loss_loc import DEGENERATE
    l = np.array([d[1] for d in DEGENERATE])
    g = np.array([d[2] for d in DEGENERATE])
    L, grad = LO.box_loss_and_grad(loc_type, l, g)
    assert np.isfinite(L).all() and np.isfinite(grad).all() and np.all(L >= 0)
