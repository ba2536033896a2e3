"""Task-aligned matching (mbx_match_tal), the parts that need no GPU: the config keys, MultiboxLoss's and Trainer's keywords,
the ctypes table, mbx_match_tal_supported, the entry's argument checks, and the numpy restatement the GPU tests compare
against (tests/tal_oracle.py) on hand-made cases with dyadic coordinates -- every value exact -- and on the cases of
tests/tal_cases.py, with the conditions those cases have to meet for the GPU tests to show anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import tal_cases as TC
from tests import tal_oracle as TO

KEY, ALPHA_KEY, BETA_KEY = "LOSS_MATCH_TAL_TOPK", "LOSS_MATCH_TAL_ALPHA", "LOSS_MATCH_TAL_BETA"
OTHERS = ("LOSS_MATCH_IOU_THRESHOLD", "LOSS_MATCH_ATSS_TOPK")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------- config keys
@pytest.mark.parametrize("cfg,want", [
    ({}, None), ({KEY: None}, None), ({KEY: None, ALPHA_KEY: None, BETA_KEY: None}, None),
    ({KEY: 13}, (13, 1.0, 6)), ({KEY: 1}, (1, 1.0, 6)), ({KEY: 45.0}, (45, 1.0, 6)), ({KEY: 2 ** 31 - 1}, (2 ** 31 - 1, 1.0, 6)),
    ({KEY: 13, ALPHA_KEY: 0}, (13, 0.0, 6)), ({KEY: 13, ALPHA_KEY: 0.5}, (13, 0.5, 6)), ({KEY: 13, ALPHA_KEY: 4}, (13, 4.0, 6)),
    ({KEY: 13, ALPHA_KEY: 2.5, BETA_KEY: 1}, (13, 2.5, 1)), ({KEY: 13, BETA_KEY: 16}, (13, 1.0, 16)),
    ({KEY: 13, BETA_KEY: 3.0}, (13, 1.0, 3)), ({KEY: 13, ALPHA_KEY: None, BETA_KEY: None}, (13, 1.0, 6))])
def test_tal_matching_accepts(cfg, want):
    from multibox_amd.config import Cfg, tal_matching, with_defaults
    for c in (Cfg(cfg), with_defaults(Cfg(cfg))):              # the defaults switch nothing on
        got = tal_matching(c)
        if want is None:
            assert got is None
        else:
            assert got == dict(tal_topk=want[0], tal_alpha=want[1], tal_beta=want[2])
            assert type(got["tal_topk"]) is int and type(got["tal_alpha"]) is float and type(got["tal_beta"]) is int


BAD = [True, False, "9", [9], float("nan"), float("inf"), -1]


@pytest.mark.parametrize("key,value", [(KEY, v) for v in BAD + [0, 2.5, 2 ** 31]] +
                         [(ALPHA_KEY, v) for v in BAD + [0.25, 1.3, 4.5, -0.5]] +
                         [(BETA_KEY, v) for v in BAD + [0, 17, 2.5]])
def test_tal_matching_rejects(key, value):
    from multibox_amd.config import Cfg, tal_matching
    cfg = {KEY: 13}
    cfg[key] = value
    with pytest.raises(ValueError, match=key):
        tal_matching(Cfg(cfg))


def test_the_exponents_only_go_with_the_topk_and_the_matching_keys_exclude_each_other():
    from multibox_amd.config import Cfg, tal_matching, atss_matching, match_iou_threshold, negative_mining, ignore_band
    for key, value in ((ALPHA_KEY, 1.0), (BETA_KEY, 6)):
        with pytest.raises(ValueError) as e:
            tal_matching(Cfg({key: value}))
        assert key in str(e.value) and KEY in str(e.value)
    for other, value in zip(OTHERS, (0.5, 9)):
        with pytest.raises(ValueError) as e:
            tal_matching(Cfg({KEY: 13, other: value}))
        assert KEY in str(e.value) and other in str(e.value)
        assert tal_matching(Cfg({KEY: 13, other: None})) == dict(tal_topk=13, tal_alpha=1.0, tal_beta=6)
        assert tal_matching(Cfg({other: value})) is None
    assert atss_matching(Cfg({KEY: 13})) is None and match_iou_threshold(Cfg({KEY: 13})) is None
    cfg = Cfg({KEY: 13, "LOSS_NEG_PER_POS": 3, "LOSS_IGNORE_IOU_THRESHOLD": 0.4, "LOSS_IGNORE_SOURCE": "prediction"})
    assert tal_matching(cfg)["tal_topk"] == 13 and negative_mining(cfg) == (3, 0)        # they compose
    assert ignore_band(cfg) == dict(ignore_iou_threshold=0.4, ignore_source="prediction")


@pytest.mark.parametrize("lines,named", [("%s: 0\n" % KEY, KEY), ("%s: 13\n%s: 0.5\n" % (KEY, OTHERS[0]), OTHERS[0]),
                                         ("%s: 13\n%s: 9\n" % (KEY, OTHERS[1]), OTHERS[1]),
                                         ("%s: 13\n%s: 0.3\n" % (KEY, ALPHA_KEY), ALPHA_KEY), ("%s: 6\n" % BETA_KEY, BETA_KEY)])
def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch, lines, named):
    import torch
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\n" + lines)

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match=named):
        train.main()


# ------------------------------------------------------------------------------------------------- MultiboxLoss, Trainer
PRIORS4 = np.array([[0, 0, .5, .5], [.25, .25, 1, 1], [0, .5, .5, 1], [.5, 0, 1, .5]], np.float32)


def test_multibox_loss_keywords_allocate_and_refuse(lib):
    import torch
    from multibox_amd import loss as L
    plain = L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu")
    assert plain.n_tal is None and plain.tal_thr is None and plain.tal_topk is None and plain.tal is None
    ml = L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=13)
    assert ml.n_tal.dtype == torch.int32 and ml.n_tal.shape == (3,)
    assert ml.tal_thr.dtype == torch.float64 and ml.tal_thr.shape == (3, 13)
    assert ml.tal_topk == 13 and ml.tal == (13, 2, 6) and ml.n_extra is None and ml.n_atss is None
    assert L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=5, tal_alpha=2.5, tal_beta=16).tal == (5, 5, 16)
    assert L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=5, tal_alpha=0, tal_beta=1).tal == (5, 0, 1)
    for bad in (0, -3, 2.5, True, "13"):
        with pytest.raises(ValueError, match="tal_topk"):
            L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=bad)
    for bad in (-0.5, 4.5, 0.25, True, "1", float("nan"), None):
        with pytest.raises(ValueError, match="tal_alpha"):
            L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=13, tal_alpha=bad)
    for bad in (0, 17, 2.5, True, "6", float("nan"), None):
        with pytest.raises(ValueError, match="tal_beta"):
            L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=13, tal_beta=bad)
    with pytest.raises(ValueError, match="tal_topk.*match_iou_threshold"):     # two matching rules
        L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=13, match_iou_threshold=0.5)
    with pytest.raises(ValueError, match="tal_topk.*atss_topk"):
        L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", tal_topk=13, atss_topk=9, prior_levels=[0, 3, 4])
    for kw in (dict(tal_alpha=0.5), dict(tal_beta=4), dict(tal_alpha=True), dict(tal_beta=None)):
        with pytest.raises(ValueError, match="without tal_topk"):              # the exponents alone
            L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", **kw)


def test_multibox_loss_refuses_a_size_the_library_refuses(lib):
    from multibox_amd import loss as L
    P, G = 4000, 300                                           # 8 P + 40 G + 64 + 2 G m: 50 KB at topk 9, 68 KB at topk 40
    assert lib.mbx_match_tal_supported(P, G, 9) == 0 and lib.mbx_match_tal_supported(P, G, 40) == -2
    priors = np.tile(PRIORS4, (P // 4, 1))
    L.MultiboxLoss(priors, 2, G, 1000.0, device="cpu", tal_topk=9)
    with pytest.raises(ValueError, match="tal_topk"):
        L.MultiboxLoss(priors, 2, G, 1000.0, device="cpu", tal_topk=40)


def test_trainer_refuses_the_same_arguments_before_it_builds_anything():
    """Trainer hands the keywords to MultiboxLoss first thing behind its one assertion on the net."""
    from multibox_amd.trainer import Trainer

    class FakeNet:
        mode, B, P, dev, heads = "train", 2, 4, "cpu", ()
    for kw, named in ((dict(tal_topk=0), "tal_topk"), (dict(tal_topk=13, tal_alpha=0.3), "tal_alpha"),
                      (dict(tal_topk=13, tal_beta=0), "tal_beta"), (dict(tal_beta=3), "without tal_topk"),
                      (dict(tal_topk=13, match_iou_threshold=0.5), "match_iou_threshold"),
                      (dict(tal_topk=13, atss_topk=9), "atss_topk")):
        with pytest.raises(ValueError, match=named):
            Trainer(FakeNet(), PRIORS4, **kw)


# ------------------------------------------------------------------------------------------------- ctypes table
def test_ctypes_signatures_have_the_argument_order_of_the_header():
    from multibox_amd import _lib
    assert {"mbx_match_tal", "mbx_match_tal_supported"} <= set(_lib.declared_symbols())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mbx.h")).read(), flags=re.S)
    want = {"mbx_match_tal": ["priors", "decoded", "conf", "gt", "n_gt", "status", "topk", "alpha_halves", "beta", "B", "P", "G",
                              "match", "n_extra", "thr", "stream"],
            "mbx_match_tal_supported": ["P", "G", "topk"]}
    for name, names in want.items():
        res, args = _lib._SIGS[name]
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m, "include/mbx.h does not declare %s" % name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names
        kind = lambda p: C.c_void_p if "*" in p or p.startswith("mbx_stream_t") else {"int": C.c_int}[p.split()[0]]
        assert res is C.c_int and args == [kind(p) for p in params]


# ------------------------------------------------------------------------------------------------- the supported envelope
def test_supported_envelope(lib):
    ok = lib.mbx_match_tal_supported
    for P, G, topk in ((646, 13, 13), (3199, 100, 13), (4221, 100, 13), (646, 13, 646)):      # the sizes the project runs
        assert ok(P, G, topk) == 0
    assert all(ok(646, 13, k) == 0 for k in range(1, 647)) and ok(646, 13, 2 ** 31 - 1) == 0  # m = min(topk, P)
    assert ok(70, 1 << 20, 4) == -2                            # more boxes than the LDS stages
    assert ok(70000, 13, 13) == -2                             # more priors than the claims in LDS hold
    # the rule of the header: 8 P + 40 G + 64 + 2 G m <= 65536, m = min(topk, P), P < 65535
    rule = lambda P, G, topk: 0 if (8 * P + 40 * G + 64 + 2 * G * min(topk, P) <= 65536 and P < 65535) else -2
    rng = np.random.RandomState(7)
    for P, G, topk in zip(rng.randint(1, 9000, 300), rng.randint(1, 1700, 300), rng.randint(1, 700, 300)):
        assert ok(int(P), int(G), int(topk)) == rule(int(P), int(G), int(topk))
    assert ok(8178, 1, 1) == 0 and ok(8179, 1, 1) == -2        # 8 P + 40 + 64 + 2 at the edge


def test_supported_argument_errors(lib):
    ok = lib.mbx_match_tal_supported
    assert ok(0, 13, 13) == -1 and ok(-5, 13, 13) == -1 and ok(646, 0, 13) == -1 and ok(646, 13, 0) == -1
    assert ok(646, 13, -9) == -1


def test_the_entry_refuses_bad_arguments_without_a_gpu(lib):
    """The argument checks come before any launch, so a host without a GPU sees them too: nothing is dereferenced and the
    buffers keep their sentinels."""
    B, P, G = 2, 70, 5
    match = np.full((B, P), -77, np.int32)
    n_extra = np.full(B, -77, np.int32)
    thr = np.full((B, G), -7.5, np.float64)
    f = np.zeros((B, P, 4), np.float32)
    z = np.zeros(B, np.int32)
    ptr = lambda a: a.ctypes.data

    def call(null=None, topk=4, halves=2, beta=6, B=B, P=P, G=G):
        p = lambda name, a: None if null == name else ptr(a)
        return lib.mbx_match_tal(p("priors", f), p("decoded", f), p("conf", f), p("gt", f), p("n_gt", z), p("status", z), topk,
                                 halves, beta, B, P, G, p("match", match), ptr(n_extra), ptr(thr), None)
    for name in ("priors", "decoded", "conf", "gt", "n_gt", "status", "match"):
        assert call(null=name) == -1
    assert call(B=-1) == -1 and call(P=0) == -1 and call(G=0) == -1 and call(topk=0) == -1
    assert call(halves=-1) == -1 and call(halves=9) == -1 and call(beta=0) == -1 and call(beta=17) == -1
    assert call(G=1 << 20) == -2 and call(P=70000) == -2
    assert call(B=0) == 0
    assert np.all(match == -77) and np.all(n_extra == -77) and np.all(thr == -7.5)


# ------------------------------------------------------------------------------------------------- the oracle, by hand
def _one(priors, decoded, conf, boxes, topk, alpha=1.0, beta=6, match=None, status=0):
    """The oracle on one image -> (match row, n_extra, thr [n])."""
    priors = np.array(priors, np.float32)
    gt = np.array([boxes], np.float32)
    m = -np.ones((1, len(priors)), np.int32) if match is None else np.array([match], np.int32)
    out, extra, thr = TO.tal(priors, np.array([decoded], np.float32), np.array([conf], np.float32), gt, [len(boxes)], [status],
                             m, topk, alpha, beta)
    return out[0].tolist(), int(extra[0]), thr[0, :len(boxes)].tolist()


QUAD = [[0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1], [.5, .5, 1, 1]]       # centres at (.25 | .75, .25 | .75)


def test_oracle_the_metric_is_the_product_of_the_powers():
    box = [0, 0, .5, .375]                                     # u = 0.75 for a prediction on prior 0
    for alpha, beta, want in ((1.0, 1, 0.5 * 0.75), (0.0, 1, 0.75), (2.0, 2, 0.25 * (0.75 * 0.75)), (0.5, 1, np.sqrt(0.5) * 0.75),
                              (1.5, 3, (0.5 * np.sqrt(0.5)) * ((0.75 * 0.75) * 0.75)), (1.0, 6, 0.5 * (0.75 ** 2 * 0.75 ** 2 * 0.75 * 0.75))):
        out, extra, thr = _one(QUAD, QUAD, [.5, .5, .5, .5], [box], 1, alpha, beta)
        assert thr == [want] and out == [0, -1, -1, -1] and extra == 1


def test_oracle_the_centre_is_the_priors_and_the_overlap_the_predictions():
    box = [0, 0, .5, .5]
    # prior 3's prediction sits on the box, but its own centre (.75, .75) is outside: no candidate
    out, extra, thr = _one(QUAD, [QUAD[1], QUAD[1], QUAD[2], QUAD[0]], [.5] * 4, [box], 4, 0.0, 1)
    assert out == [-1] * 4 and extra == 0 and thr == [0.0]    # prior 0 is inside but predicts elsewhere: t = 0
    # a centre on the edge is not inside
    assert _one([[0, 0, .5, .5]], [[0, 0, .5, .5]], [.5], [[.25, 0, .75, .5]], 1, 0.0, 1)[:2] == ([-1], 0)       # x1 == cx
    assert _one([[0, 0, .5, .5]], [[0, 0, .5, .5]], [.5], [[0, 0, .5, .25]], 1, 0.0, 1)[:2] == ([-1], 0)         # y2 == cy
    assert _one([[0, 0, .5, .5]], [[0, 0, .5, .5]], [.5], [[.125, 0, .75, .5]], 1, 0.0, 1)[:2] == ([0], 1)


def test_oracle_equal_metrics_go_to_the_lower_index_and_equal_overlaps_to_the_lower_box():
    priors = [[.25, .25, .75, .75]] * 4                        # one centre, (.5, .5)
    pred = [[.25, .25, .75, .625]] * 4                         # u = 0.75 with the box below for all four
    box = [.25, .25, .75, .75]
    out, extra, thr = _one(priors, pred, [.5, .5, .5, .5], [box], 2, 1.0, 1)
    assert out == [0, 0, -1, -1] and extra == 2 and thr == [0.375]
    out, extra, thr = _one(priors, pred, [.25, .5, .5, .75], [box], 2, 1.0, 1)
    assert out == [-1, 0, -1, 0] and thr == [0.375]            # 3 first, then the lower of 1 and 2
    # two boxes select the same prior with the same u: the lower box; a later box with a larger u wins
    out, extra, thr = _one(priors[:1], pred[:1], [.5], [[0, 0, .125, .125], box, box], 1, 0.0, 1)
    assert out == [1] and extra == 1 and thr == [0.0, 0.75, 0.75]
    out, extra, thr = _one(priors[:1], pred[:1], [.5], [box, box, pred[0]], 1, 0.0, 1)
    assert out == [2] and thr[2] == 1.0


def test_oracle_topk_over_everything_selects_exactly_the_inside_priors_with_a_positive_metric():
    for name in ("p70_all", "p646"):
        c = TC.make_case(name)
        halves = TO.alpha_halves(c["alpha"])
        for b in range(c["B"]):
            for j in range(c["n"][b]):
                picked, u, t, cand = TO.select(c["priors"], c["decoded"][b], c["conf"][b], c["gt"][b, j], c["P"], halves, c["beta"])
                with np.errstate(invalid="ignore"):
                    want = np.nonzero(TO.inside(c["priors"], c["gt"][b, j]) & (t > 0))[0]
                assert sorted(picked) == want.tolist() and np.array_equal(np.nonzero(cand)[0], want)
                assert all(t[a] >= t[b_] for a, b_ in zip(picked, picked[1:]))


def test_oracle_a_matched_prior_keeps_its_box_but_is_still_selected():
    priors = [[.25, .25, .75, .75]] * 2
    pred = [[.25, .25, .75, .75], [.25, .25, .75, .625]]       # u = 1 and 0.75
    box = [.25, .25, .75, .75]
    free = _one(priors, pred, [.5, .5], [[0, 0, .125, .125], box], 1, 0.0, 1)
    held = _one(priors, pred, [.5, .5], [[0, 0, .125, .125], box], 1, 0.0, 1, match=[0, -1])
    assert free == ([1, -1], 1, [0.0, 1.0])
    assert held == ([0, -1], 0, [0.0, 1.0])                    # prior 0 takes the one place and keeps box 0: prior 1 stays free


def test_oracle_skips_and_padding():
    c = TC.make_case("p70")
    full, full_extra, full_thr = TC.oracle("p70")
    args = lambda **kw: [kw.get(k, c[k]) for k in ("priors", "decoded", "conf", "gt", "n", "status", "match")] + \
        [c["topk"], c["alpha"], c["beta"]]
    st = np.array([0, 1, 2, 0], np.int32)
    out, extra, thr = TO.tal(*args(status=st))
    assert np.array_equal(out[[0, 1, 2]], c["match"][[0, 1, 2]]) and extra[:3].tolist() == [0, 0, 0] and not thr[:3].any()
    assert np.array_equal(out[3], full[3]) and extra[3] == full_extra[3] and np.array_equal(thr[3], full_thr[3])
    n = c["n"].copy()
    n[1] = c["G"] + 1
    out, extra, thr = TO.tal(*args(n=n))
    assert np.array_equal(out[1], c["match"][1]) and extra[1] == 0 and not thr[1].any()
    nan_pad = c["gt"].copy()
    for b in range(c["B"]):
        nan_pad[b, c["n"][b]:] = np.nan
    again = TO.tal(*args(gt=nan_pad))
    assert all(np.array_equal(x, y) for x, y in zip(again, (full, full_extra, full_thr)))


def test_oracle_a_nan_prediction_is_never_selected():
    c = TC.make_case("p70")
    full, _, _ = TC.oracle("p70")
    added = np.argwhere((full >= 0) & (c["match"] < 0))
    assert len(added) >= 8
    decoded, conf = c["decoded"].copy(), c["conf"].copy()
    hit = added[:8]
    for i, (b, p) in enumerate(hit[:4]):
        decoded[b, p, i] = np.nan                              # one corner each
    for b, p in hit[4:6]:
        decoded[b, p] = np.nan
    for b, p in hit[6:8]:
        conf[b, p] = np.nan
    out, extra, thr = TO.tal(c["priors"], decoded, conf, c["gt"], c["n"], c["status"], c["match"], c["topk"], c["alpha"], c["beta"])
    for b, p in hit:
        assert out[b, p] == -1
    assert not np.isnan(thr).any()
    halves = TO.alpha_halves(c["alpha"])
    for b in range(c["B"]):
        for j in range(c["n"][b]):
            picked = TO.select(c["priors"], decoded[b], conf[b], c["gt"][b, j], c["P"], halves, c["beta"])[0]
            assert not any((b, p) in {tuple(h) for h in hit} for p in picked)


# ------------------------------------------------------------------------------------------------- the oracle, on the cases
@pytest.mark.parametrize("name", list(TC.CASES))
def test_the_two_formulations_agree(name):
    c = TC.make_case(name)
    other = TO.tal_sorted(c["priors"], c["decoded"], c["conf"], c["gt"], c["n"], c["status"], c["match"], c["topk"], c["alpha"],
                          c["beta"])
    for x, y in zip(TC.oracle(name), other):
        assert x.tobytes() == y.tobytes()


@pytest.fixture(scope="module")
def survey():
    """Per case what it exercises: the candidates per box, boxes with equal t at ranks topk and topk + 1, free priors that
    at least two boxes selected, selected priors that were already matched, and the most one lane (prior index mod 64) hands
    out for a box with more candidates than topk."""
    res = {}
    for name in TC.CASES:
        c = TC.make_case(name)
        halves = TO.alpha_halves(c["alpha"])
        cands, ties, shared, held, deepest = [], 0, 0, 0, 0
        for b in range(c["B"]):
            times = np.zeros(c["P"], int)
            for j in range(c["n"][b]):
                picked, u, t, cand = TO.select(c["priors"], c["decoded"][b], c["conf"][b], c["gt"][b, j], c["topk"], halves, c["beta"])
                cands.append(int(cand.sum()))
                assert len(picked) == min(c["topk"], cands[-1])
                ranked = np.sort(t[cand])[::-1]
                if len(ranked) > c["topk"]:
                    ties += int(ranked[c["topk"] - 1] == ranked[c["topk"]])
                    deepest = max(deepest, int(np.bincount(np.array(picked) % 64).max()))
                for p in picked:
                    if c["match"][b, p] < 0:
                        times[p] += 1
                    else:
                        held += 1
            shared += int((times >= 2).sum())
        res[name] = dict(cands=cands, ties=ties, shared=shared, held=held, deepest=deepest)
        print(name, "topk", c["topk"], "candidates", min(cands), "to", max(cands), "ties at the cut", ties, "shared", shared,
              "selected but held", held, "most from one lane", deepest)
    return res


@pytest.mark.parametrize("name", list(TC.CASES))
def test_oracle_properties_on_the_gpu_cases(name):
    c = TC.make_case(name)
    out, n_extra, thr = TC.oracle(name)
    assert (c["B"], c["P"], c["G"]) == c["match"].shape + (c["gt"].shape[1],) and c["decoded"].shape == (c["B"], c["P"], 4)
    assert c["conf"].dtype == np.float32 and c["conf"].min() > 0.01 - 1e-6 and c["conf"].max() < 0.99 + 1e-6
    assert c["n"][0] == 0 and c["n"][-1] == min(c["G"], c["P"])
    assert n_extra.sum() >= 1 and n_extra[0] == 0             # every case adds at least one prior, its image 0 none
    had = c["match"] >= 0
    assert had.any() and np.array_equal(out[had], c["match"][had])             # a matched prior is never reassigned
    assert np.array_equal(n_extra, ((out >= 0) & ~had).sum(1))
    halves = TO.alpha_halves(c["alpha"])
    for b in range(c["B"]):
        assert not thr[b, c["n"][b]:].any() and (out[b] < max(c["n"][b], 1)).all()
        for j in range(c["n"][b]):
            picked, u, t, cand = TO.select(c["priors"], c["decoded"][b], c["conf"][b], c["gt"][b, j], c["topk"], halves, c["beta"])
            assert thr[b, j] == (t[picked[-1]] if picked else 0.0)
            for p in np.nonzero((out[b] == j) & ~had[b])[0]:                   # every added prior was selected by its box
                assert p in picked


def test_the_cases_meet_the_conditions_the_gpu_tests_rest_on(survey):
    fewer = any(n < TC.make_case(name)["topk"] for name, s in survey.items() for n in s["cands"])
    more = any(n > TC.make_case(name)["topk"] for name, s in survey.items() for n in s["cands"])
    assert fewer and more                                      # some box has fewer candidates than topk, some box more
    assert survey["p70_lattice"]["ties"] >= 1                  # equal t at ranks topk and topk + 1
    assert survey["p646"]["shared"] >= 1 or survey["p3199"]["shared"] >= 1     # a free prior selected by two boxes
    assert any(s["held"] >= 1 for s in survey.values())        # a selected prior that was already matched
    assert all(n <= TC.make_case("p70_all")["topk"] for n in survey["p70_all"]["cands"])      # all selected: no round
    assert survey["p646_deep"]["deepest"] > 4                  # a lane hands out more than the four it keeps: it scans again
    assert survey["p3199"]["cands"] and TC.make_case("p3199")["n"][-1] == 100  # 100 boxes on 16 wavefronts: boxes in a row
