"""The ignore band (mbx_match_ignore, mbx_loss_fwd_bwd_ignore), the parts that need no GPU: the config keys, the keyword
arguments of MultiboxLoss, the numpy restatements the GPU tests compare against (tests/ignore_oracle.py) on hand-made cases
and on the GPU tests' own cases, and the ctypes table."""
import os
import re

import numpy as np
import pytest

from tests import extend_oracle as EO
from tests import ignore_oracle as IO

KEY, SOURCE, MATCH_KEY = "LOSS_IGNORE_IOU_THRESHOLD", "LOSS_IGNORE_SOURCE", "LOSS_MATCH_IOU_THRESHOLD"


# ------------------------------------------------------------------------------------------------- config keys
@pytest.mark.parametrize("cfg,want", [
    ({}, None),
    ({KEY: None}, None),
    ({KEY: None, SOURCE: None}, None),
    ({KEY: 0.4}, {"ignore_iou_threshold": 0.4, "ignore_source": "prior"}),
    ({KEY: 1}, {"ignore_iou_threshold": 1.0, "ignore_source": "prior"}),
    ({KEY: 1e-3, SOURCE: "prior"}, {"ignore_iou_threshold": 1e-3, "ignore_source": "prior"}),
    ({KEY: 0.7, SOURCE: "prediction"}, {"ignore_iou_threshold": 0.7, "ignore_source": "prediction"}),
    ({KEY: 0.4, MATCH_KEY: 0.5}, {"ignore_iou_threshold": 0.4, "ignore_source": "prior"}),
    ({KEY: 0.5, MATCH_KEY: 0.5}, {"ignore_iou_threshold": 0.5, "ignore_source": "prior"}),      # the band is the one IoU 0.5
    ({KEY: 0.7, MATCH_KEY: 0.5, SOURCE: "prediction"}, {"ignore_iou_threshold": 0.7, "ignore_source": "prediction"}),
    ({KEY: 0.4, "LOSS_MATCH_ATSS_TOPK": 9, "LOSS_NEG_PER_POS": 3, "LOSS_QUALITY_TARGET": "qfl", "LOSS_LOC_TYPE": "giou"},
     {"ignore_iou_threshold": 0.4, "ignore_source": "prior"}),
    ({KEY: 0.4, "LOSS_FOCAL_GAMMA": 2.0}, {"ignore_iou_threshold": 0.4, "ignore_source": "prior"}),
])
def test_ignore_band_accepts(cfg, want):
    from multibox_amd.config import DEFAULTS, Cfg, ignore_band, with_defaults
    assert ignore_band(Cfg(cfg)) == want
    got = ignore_band(with_defaults(Cfg(cfg)))                # the defaults switch nothing on
    assert got == want and (got is None or type(got["ignore_iou_threshold"]) is float)
    assert KEY not in DEFAULTS and SOURCE not in DEFAULTS


@pytest.mark.parametrize("value", [0, 0.0, -0.1, 1.5, 2, True, False, "0.4", [0.4], float("nan"), float("inf")])
def test_ignore_band_rejects_the_threshold(value):
    from multibox_amd.config import Cfg, ignore_band
    with pytest.raises(ValueError, match=KEY):
        ignore_band(Cfg({KEY: value}))


@pytest.mark.parametrize("value", ["priors", "", 1, True, ["prior"], 0.5])
def test_ignore_band_rejects_the_source(value):
    from multibox_amd.config import Cfg, ignore_band
    with pytest.raises(ValueError, match=SOURCE):
        ignore_band(Cfg({KEY: 0.4, SOURCE: value}))


def test_the_source_without_the_threshold_and_the_empty_band_are_errors():
    from multibox_amd.config import Cfg, ignore_band
    with pytest.raises(ValueError, match=SOURCE):
        ignore_band(Cfg({SOURCE: "prediction"}))
    with pytest.raises(ValueError, match=SOURCE):
        ignore_band(Cfg({SOURCE: "prior"}))
    with pytest.raises(ValueError) as e:
        ignore_band(Cfg({KEY: 0.6, MATCH_KEY: 0.5}))
    assert KEY in str(e.value) and MATCH_KEY in str(e.value)
    with pytest.raises(ValueError, match=MATCH_KEY):           # a bad matching threshold is still named
        ignore_band(Cfg({KEY: 0.4, MATCH_KEY: 1.5}))


def test_the_other_keys_do_not_see_these():
    from multibox_amd import config as CF
    cfg = CF.Cfg({KEY: 0.4, SOURCE: "prediction"})
    assert CF.negative_mining(cfg) is None and CF.match_iou_threshold(cfg) is None and CF.atss_matching(cfg) is None
    assert CF.focal_loss(cfg) is None and CF.loc_loss(cfg) is None and CF.quality_loss(cfg) is None


def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch):
    import torch
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\n%s: 0.6\n%s: 0.5\n" % (KEY, MATCH_KEY))

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match=KEY):
        train.main()


# ------------------------------------------------------------------------------------------------- MultiboxLoss
PRIORS = np.array([[0, 0, .5, .5], [.25, .25, 1, 1]], np.float32)


def test_multibox_loss_keywords_allocate_n_ignored_and_choose_the_entry():
    import torch
    import __graft_entry__ as g
    g.build()                                                 # the constructor asks the library for its workspace size
    from multibox_amd import loss as L
    off = L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu")
    assert off.n_ignored is None and off.ignore is None and off.entry == "mbx_loss_fwd_bwd" and off.entry_args == ()
    assert L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", neg_per_pos=3).entry == "mbx_loss_fwd_bwd_mined"
    ml = L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=0.4)
    assert ml.n_ignored.dtype == torch.int32 and ml.n_ignored.shape == (3,) and ml.ignore == (0.4, 0)
    assert ml.entry == "mbx_loss_fwd_bwd_ignore" and ml.q_stats is None and ml.n_neg is None
    # loc_type, loc_beta | quality, gamma, w_pos, w_neg | neg_per_pos, min_neg, n_neg | q_stats: the plain loss through the superset
    assert ml.entry_args == (0, 0.0, 0, 0.0, 1.0, 1.0, 0, 0, None, None)
    ml = L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=0.4, ignore_source="prediction",
                        focal_gamma=2.0, focal_alpha=0.25, loc_loss="smooth_l1", neg_per_pos=3, min_neg=2)
    assert ml.ignore == (0.4, 1) and ml.entry == "mbx_loss_fwd_bwd_ignore"
    assert ml.entry_args == (1, L.LOC_BETA_DEFAULT, 0, 2.0, 0.25, 0.75, 3, 2, ml.n_neg.data_ptr(), None)
    ml = L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=1, quality_target="varifocal", loc_loss="giou")
    assert ml.entry == "mbx_loss_fwd_bwd_ignore" and ml.q_stats.shape == (3, 2) and ml.q_stats.dtype == torch.float64
    assert ml.entry_args == (2, 0.0, 2, 2.0, 1.0, 0.75, 0, 0, None, ml.q_stats.data_ptr())
    ml = L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=0.5, match_iou_threshold=0.5)
    assert ml.n_extra is not None and ml.n_ignored is not None


def test_multibox_loss_refuses_bad_values():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import loss as L
    for bad in (0, 1.5, float("nan"), True, "0.4", -0.1, 1e-60):      # 1e-60 is 0 as the float32 the entry takes
        with pytest.raises(ValueError, match="ignore_iou_threshold"):
            L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=bad)
    for bad in ("priors", None, 1):
        with pytest.raises(ValueError, match="ignore_source"):
            L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=0.4, ignore_source=bad)
    with pytest.raises(ValueError, match="ignore_source"):
        L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_source="prediction")
    with pytest.raises(ValueError) as e:
        L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=0.6, match_iou_threshold=0.5)
    assert "ignore_iou_threshold" in str(e.value) and "match_iou_threshold" in str(e.value)
    # by the prediction's overlap the two thresholds judge different boxes: no empty band to refuse
    L.MultiboxLoss(PRIORS, 3, 13, 1000.0, device="cpu", ignore_iou_threshold=0.6, match_iou_threshold=0.5,
                   ignore_source="prediction")


# ------------------------------------------------------------------------------------------------- the match oracle
HALF = np.array([[[0, 0, .5, .25]]], np.float32)              # IoU exactly 0.5 with PRIORS[0], 0 with PRIORS[1]


def test_an_iou_of_exactly_the_threshold_is_ignored():
    free = -np.ones((1, 2), np.int32)
    assert EO.iou_row(PRIORS[0], HALF[0])[0] == 0.5 and EO.iou_row(PRIORS[1], HALF[0])[0] == 0.0
    out, n = IO.ignore(PRIORS, 0, HALF, [1], [0], free, 0.5)
    assert out.tolist() == [[-2, -1]] and n.tolist() == [1]   # not strict
    above = np.nextafter(np.float32(0.5), np.float32(1))
    out, n = IO.ignore(PRIORS, 0, HALF, [1], [0], free, above)
    assert out.tolist() == [[-1, -1]] and n.tolist() == [0]
    # mbx_match_extend at the same threshold takes what is over it: the two never claim the same prior
    ext, _ = EO.extend(PRIORS, HALF, [1], [0], free, 0.5)
    assert ext.tolist() == [[-1, -1]]


def test_per_image_boxes_a_nan_box_and_what_is_left_alone():
    gt = np.array([[[0, 0, .5, .5], [.5, .5, 1, 1]], [[0, 0, .5, .5], [0, 0, 0, 0]]], np.float32)
    boxes = np.array([[[0, 0, .5, .5], [.5, .5, 1, 1], [np.nan, 0, .5, .5], [0, 0, .5, .5], [0, 0, .5, .5], [.5, 0, 0, .5]],
                      [[.5, .5, 1, 1], [0, 0, .5, .5], [0, 0, .5, .5], [0, 0, np.inf, .5], [0, 0, .5, .5], [0, 0, .5, .5]]],
                     np.float32)
    match = np.array([[-1, -1, -1, 0, -3, -1], [-1, -1, -2, -1, -77, 1]], np.int32)
    out, n = IO.ignore(boxes, 1, gt, [2, 1], [0, 0], match, 1.0)
    # image 0: IoU 1 with box 0, with box 1, a NaN box passes nothing, a positive stays, -3 stays, an inverted box has iw < 0
    # image 1 (one box): its own row of boxes -- prior 0 is off the box, 1 is on it, -2 stays (and is not counted again),
    # an infinite box has uni = inf and IoU 0, -77 stays, a positive stays
    assert out.tolist() == [[-2, -2, -1, 0, -3, -1], [-1, -2, -2, -1, -77, 1]] and n.tolist() == [2, 1]
    again, n2 = IO.ignore(boxes, 1, gt, [2, 1], [0, 0], out, 1.0)
    assert np.array_equal(again, out) and n2.tolist() == [0, 0]                 # idempotent
    shared, n3 = IO.ignore(boxes[0], 0, gt, [2, 1], [0, 0], match, 1.0)         # image 0's boxes for both images
    assert shared.tolist() == [[-2, -2, -1, 0, -3, -1], [-2, -1, -2, -2, -77, 1]] and n3.tolist() == [2, 2]


def test_skipped_images_and_padding():
    gt = np.tile(np.array([[0, 0, .5, .5], [np.nan] * 4], np.float32), (4, 1, 1))
    match = -np.ones((4, 2), np.int32)
    out, n = IO.ignore(PRIORS, 0, gt, [1, 0, 1, 3], [0, 0, 2, 0], match, 0.9)
    assert out.tolist() == [[-2, -1], [-1, -1], [-1, -1], [-1, -1]] and n.tolist() == [1, 0, 0, 0]   # n = 0, status, n > G
    out, n = IO.ignore(PRIORS, 0, gt, [2, 0, 1, 3], [0, 0, 2, 0], match, 0.9)   # the NaN row read: it passes nothing
    assert out.tolist()[0] == [-2, -1] and n[0] == 1


# (B, P, G) -> the number ignored per image on the hand-made match at 0.5, and behind the oracle's extend at 0.5 with 0.3
CENSUS = {(3, 13, 13): ([0, 6, 2], [0, 0, 0]), (4, 70, 5): ([0, 7, 3, 1], [0, 2, 3, 0]),
          (4, 646, 13): ([0, 47, 3, 17], [0, 129, 5, 51]), (2, 3199, 100): ([0, 966], [0, 1504])}


@pytest.mark.parametrize("B,P,G", sorted(CENSUS))
def test_the_gpu_tests_cases_ignore_what_they_are_said_to_and_the_band_is_the_complement(B, P, G):
    from tests.test_gpu_match_extend import make_case
    c = make_case(B, P, G)
    out, n = IO.ignore(c["priors"], 0, c["gt"], c["n"], c["status"], c["match"], 0.5)
    assert n.tolist() == CENSUS[(B, P, G)][0]
    assert np.array_equal(out[c["match"] != -1], c["match"][c["match"] != -1])
    ext, _ = EO.extend(c["priors"], c["gt"], c["n"], c["status"], c["match"], 0.5)
    band, n = IO.ignore(c["priors"], 0, c["gt"], c["n"], c["status"], ext, 0.3)
    assert n.tolist() == CENSUS[(B, P, G)][1]
    best = IO.best_iou(c["priors"], c["gt"], c["n"])
    lo, hi = float(np.float32(0.3)), float(np.float32(0.5))
    free = c["match"] < 0
    assert np.array_equal(band == -2, free & (best >= lo) & (best <= hi))       # no gap
    assert np.array_equal(band >= 0, ~free | (best > hi))                       # no overlap: what extend took is not ignored


# ------------------------------------------------------------------------------------------------- the loss oracle
def test_loss_oracle_is_the_quality_oracle_without_ignored_priors_and_compacts_with_them():
    from tests import loc_oracle as LO
    from tests import quality_oracle as QO
    c = LO.make_loc_case(4, 70, 5)
    args = ("giou", c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, 2.0, 1.0, 0.75, 3, 2)
    ref, got = QO.quality_loss("qfl", *args), IO.loss("qfl", *args)
    assert np.array_equal(got["n_neg"], ref["n_neg"]) and np.array_equal(got["d_conf_in"], ref["d_conf_in"])
    assert np.array_equal(got["dl"], ref["dl"]) and np.array_equal(got["q_stats"], ref["q_stats"])
    assert np.isclose(got["conf_loss"], ref["conf_loss"], rtol=1e-13) and np.isclose(got["loc_loss"], ref["loc_loss"], rtol=1e-13)
    # the selected negatives of image 2 ignored: the budget stays (positives unchanged) and goes to the next ones
    match = c["match"].copy()
    taken = np.nonzero((match[2] < 0) & ref["mask"][2])[0]
    assert taken.size >= 3
    match[2, taken] = -2
    got = IO.loss("qfl", *(args[:5] + (match,) + args[6:]))
    assert got["n_neg"][2] == ref["n_neg"][2] and np.all(got["d_conf_in"][2, taken] == 0)
    newly = (got["d_conf_in"][2] != 0) & (ref["d_conf_in"][2] == 0)
    assert newly.sum() == taken.size and not (match[2][newly] >= 0).any()
    assert np.array_equal(got["d_conf_in"][[0, 1, 3]], ref["d_conf_in"][[0, 1, 3]])
    # every free prior ignored: K = 0, the positives alone
    match = np.where(c["match"] < 0, -2, c["match"]).astype(np.int32)
    got = IO.loss("varifocal", *(args[:5] + (match,) + args[6:]))
    assert not got["n_neg"].any() and np.all(got["d_conf_in"][match < 0] == 0)
    assert np.array_equal(got["q_stats"], ref["q_stats"])
    # without a quality target: the focal oracle on what is left
    got = IO.loss(None, *(args[:5] + (c["match"],) + args[6:]))
    want = LO.loc_loss("giou", c["dec"], c["z"], 1, c["gt"], c["match"], 1000.0, LO.BETA, 2.0, 1.0, 0.75, 3, 2)
    assert np.array_equal(got["d_conf_in"], want["d_conf_in"]) and np.array_equal(got["n_neg"], want["n_neg"])


# ------------------------------------------------------------------------------------------------- ctypes table
@pytest.mark.parametrize("name,names", [
    ("mbx_match_ignore", ["boxes", "per_image", "gt", "n_gt", "status", "iou_threshold", "B", "P", "G", "match", "n_ignored",
                          "stream"]),
    ("mbx_loss_fwd_bwd_ignore", None)])
def test_ctypes_signatures_have_the_argument_order_of_the_header(name, names):
    import ctypes as C
    from multibox_amd import _lib
    assert name in _lib.declared_symbols()
    res, args = _lib._SIGS[name]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mbx.h")).read(), flags=re.S)
    params = {}
    for fn in (name, "mbx_loss_fwd_bwd_quality"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % fn, hdr)
        assert m, "include/mbx.h does not declare %s" % fn
        params[fn] = [" ".join(p.split()) for p in m.group(1).split(",")]
    if names is None:                                         # mbx_loss_fwd_bwd_quality's arguments, same order
        assert params[name] == params["mbx_loss_fwd_bwd_quality"] and args == _lib._SIGS["mbx_loss_fwd_bwd_quality"][1]
    else:
        assert [p.split()[-1].lstrip("*") for p in params[name]] == names
    kind = lambda p: C.c_void_p if "*" in p or p.startswith("mbx_stream_t") else \
        {"float": C.c_float, "int": C.c_int, "size_t": C.c_size_t}[p.split()[0]]
    assert res is C.c_int and args == [kind(p) for p in params[name]]
    assert re.search(r"MBX_MATCH_FREE\s*=\s*-1\s*,\s*MBX_MATCH_IGNORED\s*=\s*-2", hdr)
