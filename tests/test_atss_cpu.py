"""ATSS matching (mbx_match_atss), the parts that need no GPU: the config key, MultiboxLoss's keywords, the ctypes table,
mbx_match_atss_supported, and the numpy restatement the GPU tests compare against (tests/atss_oracle.py) on hand-made cases
with dyadic coordinates -- every value exact -- and on the cases of tests/atss_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import atss_cases as AC
from tests import atss_oracle as AO

KEY, OTHER = "LOSS_MATCH_ATSS_TOPK", "LOSS_MATCH_IOU_THRESHOLD"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------- config key
@pytest.mark.parametrize("cfg,want", [({}, None), ({KEY: None}, None), ({KEY: 1}, 1), ({KEY: 9}, 9), ({KEY: 45.0}, 45),
                                      ({KEY: 2 ** 31 - 1}, 2 ** 31 - 1)])
def test_atss_matching_accepts(cfg, want):
    from multibox_amd.config import Cfg, atss_matching, with_defaults
    assert atss_matching(Cfg(cfg)) == want
    got = atss_matching(with_defaults(Cfg(cfg)))               # the defaults switch nothing on
    assert got == want and (got is None or type(got) is int)


@pytest.mark.parametrize("value", [True, False, 0, -1, 2.5, "9", [9], float("nan"), float("inf"), 2 ** 31])
def test_atss_matching_rejects(value):
    from multibox_amd.config import Cfg, atss_matching
    with pytest.raises(ValueError, match=KEY):
        atss_matching(Cfg({KEY: value}))


def test_the_two_matching_keys_do_not_go_together():
    from multibox_amd.config import Cfg, atss_matching, match_iou_threshold, negative_mining
    with pytest.raises(ValueError) as e:
        atss_matching(Cfg({KEY: 9, OTHER: 0.5}))
    assert KEY in str(e.value) and OTHER in str(e.value)
    assert atss_matching(Cfg({KEY: 9, OTHER: None})) == 9
    assert atss_matching(Cfg({OTHER: 0.5})) is None and match_iou_threshold(Cfg({KEY: 9})) is None
    cfg = Cfg({KEY: 9, "LOSS_NEG_PER_POS": 3})                 # mining does not see it, nor it mining
    assert atss_matching(cfg) == 9 and negative_mining(cfg) == (3, 0)


@pytest.mark.parametrize("lines", ["%s: 0\n" % KEY, "%s: 9\n%s: 0.5\n" % (KEY, OTHER)])
def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch, lines):
    import torch
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\n" + lines)

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match=KEY):
        train.main()


# ------------------------------------------------------------------------------------------------- MultiboxLoss
PRIORS4 = np.array([[0, 0, .5, .5], [.25, .25, 1, 1], [0, .5, .5, 1], [.5, 0, 1, .5]], np.float32)


def test_multibox_loss_keywords_allocate_and_refuse(lib):
    import torch
    from multibox_amd import loss as L
    plain = L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu")
    assert plain.n_atss is None and plain.atss_thr is None and plain.atss_topk is None
    ml = L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", atss_topk=9, prior_levels=[0, 3, 4])
    assert ml.n_atss.dtype == torch.int32 and ml.n_atss.shape == (3,)
    assert ml.atss_thr.dtype == torch.float64 and ml.atss_thr.shape == (3, 13)
    assert ml.atss_topk == 9 and ml.prior_levels == [0, 3, 4] and ml.n_extra is None
    with pytest.raises(ValueError, match="prior_levels"):                      # missing
        L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", atss_topk=9)
    for bad in ([0, 3], [1, 4], [0, 2, 2, 4], [0, 3, 2, 4], [0, 1, 2, 3, 4, 5], list(range(0, 5)) + [9] * 6, "levels", [0, None]):
        with pytest.raises(ValueError, match="prior_levels"):                  # malformed
            L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", atss_topk=9, prior_levels=bad)
    for bad in (0, -3, 2.5, True, "9"):
        with pytest.raises(ValueError, match="atss_topk"):
            L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", atss_topk=bad, prior_levels=[0, 3, 4])
    with pytest.raises(ValueError, match="atss_topk.*match_iou_threshold"):    # both matching rules
        L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", atss_topk=9, prior_levels=[0, 3, 4], match_iou_threshold=0.5)
    with pytest.raises(ValueError, match="prior_levels"):
        L.MultiboxLoss(PRIORS4, 3, 13, 1000.0, device="cpu", prior_levels=[0, 3, 4])


def test_multibox_loss_refuses_a_size_the_library_refuses(lib):
    from multibox_amd import loss as L
    P, G = 4000, 300                                           # topk 40 on two levels: 8 P + 40 G + 2 G m alone is over 64 KB
    levels = (C.c_int32 * 3)(0, 2000, P)
    assert lib.mbx_match_atss_supported(P, G, 2, levels, 9) == 0 and lib.mbx_match_atss_supported(P, G, 2, levels, 40) == -2
    priors = np.tile(PRIORS4, (P // 4, 1))
    L.MultiboxLoss(priors, 2, G, 1000.0, device="cpu", atss_topk=9, prior_levels=[0, 2000, P])
    with pytest.raises(ValueError, match="atss_topk"):
        L.MultiboxLoss(priors, 2, G, 1000.0, device="cpu", atss_topk=40, prior_levels=[0, 2000, P])


# ------------------------------------------------------------------------------------------------- ctypes table
def test_ctypes_signatures_have_the_argument_order_of_the_header():
    from multibox_amd import _lib
    assert {"mbx_match_atss", "mbx_match_atss_supported"} <= set(_lib.declared_symbols())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mbx.h")).read(), flags=re.S)
    want = {"mbx_match_atss": ["priors", "level_start", "n_levels", "gt", "n_gt", "status", "topk", "B", "P", "G", "match",
                               "n_extra", "thr", "stream"],
            "mbx_match_atss_supported": ["P", "G", "n_levels", "level_start", "topk"]}
    for name, names in want.items():
        res, args = _lib._SIGS[name]
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m, "include/mbx.h does not declare %s" % name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names
        kind = lambda p: C.c_void_p if "*" in p or p.startswith("mbx_stream_t") else {"int": C.c_int}[p.split()[0]]
        assert res is C.c_int and args == [kind(p) for p in params]


# ------------------------------------------------------------------------------------------------- the supported envelope
def _levels(*v):
    return (C.c_int32 * len(v))(*v)


def test_supported_envelope(lib):
    ok = lib.mbx_match_atss_supported
    assert ok(3199, 100, 6, _levels(*AC.LEVELS_512), 9) == 0
    l299 = _levels(*AC.LEVELS_299)
    assert all(ok(646, 13, 6, l299, k) == 0 for k in range(1, 647))
    assert ok(4221, 100, 6, _levels(0, 1800, 3100, 3600, 3900, 4150, 4221), 9) == 0          # mbx_match's own limit
    assert ok(646, 13, 6, l299, 2 ** 31 - 1) == 0                                            # topk over every level: all of it


def test_supported_argument_errors(lib):
    ok = lib.mbx_match_atss_supported
    l299 = _levels(*AC.LEVELS_299)
    assert ok(9, 13, 9, _levels(*range(10)), 9) == -1          # nine levels
    assert ok(8, 13, 8, _levels(*range(9)), 9) == 0            # eight are fine
    assert ok(646, 13, 0, l299, 9) == -1
    assert ok(647, 13, 6, l299, 9) == -1                       # the table does not end at P
    assert ok(646, 13, 6, _levels(1, 320, 500, 580, 625, 645, 646), 9) == -1      # does not start at 0
    assert ok(646, 13, 6, _levels(0, 320, 320, 580, 625, 645, 646), 9) == -1      # not strictly ascending
    assert ok(646, 13, 6, _levels(0, 500, 320, 580, 625, 645, 646), 9) == -1
    assert ok(646, 13, 6, l299, 0) == -1 and ok(646, 13, 6, l299, -9) == -1
    assert ok(646, 0, 6, l299, 9) == -1 and ok(0, 13, 1, _levels(0, 0), 9) == -1
    assert ok(646, 13, 6, None, 9) == -1
    assert ok(70000, 13, 1, _levels(0, 70000), 9) == -2        # more priors than the claims in LDS hold
    assert ok(646, 5000, 6, l299, 9) == -2                     # more boxes


def test_the_entry_refuses_bad_arguments_without_a_gpu(lib):
    """The argument checks come before any launch, so a host without a GPU sees them too: nothing is dereferenced."""
    l299 = _levels(*AC.LEVELS_299)
    one = C.c_void_p(8)                                        # a non-NULL pointer that is never followed
    call = lambda levels=l299, n_levels=6, topk=9, B=1, P=646, G=13, priors=one, match=one: lib.mbx_match_atss(
        priors, levels, n_levels, one, one, one, topk, B, P, G, match, None, None, None)
    assert call(priors=None) == -1 and call(match=None) == -1 and call(levels=None) == -1
    assert call(B=-1) == -1 and call(topk=0) == -1 and call(n_levels=9) == -1 and call(P=645) == -1
    assert call(G=5000) == -2
    assert call(B=0) == 0


# ------------------------------------------------------------------------------------------------- the oracle, by hand
def _one(priors, levels, boxes, topk, match=None, status=0):
    """The oracle on one image -> (match row, n_extra, thr [n])."""
    priors = np.array(priors, np.float32)
    gt = np.array([boxes], np.float32)
    m = -np.ones((1, len(priors)), np.int32) if match is None else np.array([match], np.int32)
    out, extra, thr = AO.atss(priors, levels, gt, [len(boxes)], [status], m, topk)
    return out[0].tolist(), int(extra[0]), thr[0, :len(boxes)].tolist()


def test_oracle_one_candidate_is_its_own_threshold():
    # one level, topk 1: m = 1, std = 0, thr = the candidate's IoU, and >= makes it a positive
    priors = [[0, 0, .5, .5], [.5, .5, 1, 1]]
    out, extra, thr = _one(priors, [0, 2], [[0, 0, .5, .375]], 1)
    assert thr == [0.75] and out == [0, -1] and extra == 1


def test_oracle_a_centre_on_the_box_edge_is_not_inside():
    priors = [[0, 0, .5, .5]]                                  # centre (.25, .25)
    assert _one(priors, [0, 1], [[.25, 0, .75, .5]], 1) == ([-1], 0, [0.5 * .25 / (.25 + .25 - .125)])    # x1 == cx
    assert _one(priors, [0, 1], [[0, 0, .25, .5]], 1)[:2] == ([-1], 0)                                     # x2 == cx
    assert _one(priors, [0, 1], [[0, .25, .5, .75]], 1)[:2] == ([-1], 0)                                   # y1 == cy
    assert _one(priors, [0, 1], [[0, 0, .5, .25]], 1)[:2] == ([-1], 0)                                     # y2 == cy
    assert _one(priors, [0, 1], [[.125, 0, .75, .5]], 1)[:2] == ([0], 1)                                   # just inside


def test_oracle_equal_claims_go_to_the_lower_box_and_a_larger_iou_wins():
    priors = [[.25, .25, .75, .75]]
    box = [.25, .25, .75, .5 + .125]                           # IoU 0.75, the centre (.5, .5) inside
    out, extra, thr = _one(priors, [0, 1], [[0, 0, .125, .125], box, box], 1)
    assert thr == [0.0, 0.75, 0.75] and out == [1] and extra == 1              # 1 and 2 are equal: 1
    out, extra, thr = _one(priors, [0, 1], [box, box, [.25, .25, .75, .75]], 1)
    assert thr[2] == 1.0 and out == [2] and extra == 1                         # a later box with a larger IoU wins


def test_oracle_iou_zero_at_threshold_zero_stays_free():
    out, extra, thr = _one([[0, 0, .25, .25]], [0, 1], [[.5, .5, 1, 1]], 1)
    assert thr == [0.0] and out == [-1] and extra == 0


def test_oracle_equal_distances_across_the_cut_go_to_the_lower_index():
    # four priors at the same distance from the box centre (.5, .5); topk 2 takes 0 and 1
    priors = [[.25, .25, .5, .5], [.5, .25, .75, .5], [.25, .5, .5, .75], [.5, .5, .75, .75]]
    box = [.25, .25, .75, .75]
    assert len(set(AO.distances(np.array(priors, np.float32), np.array(box, np.float32)).tolist())) == 1
    assert AO.candidates(np.array(priors, np.float32), [0, 4], np.array(box, np.float32), 2) == [0, 1]
    assert AO.candidates(np.array(priors, np.float32), [0, 4], np.array(box, np.float32), 3) == [0, 1, 2]
    out, extra, thr = _one(priors, [0, 4], [box], 2)
    assert thr == [0.25] and out == [0, 0, -1, -1] and extra == 2              # every IoU is 0.25: std 0, thr 0.25
    # a NaN distance ranks behind +inf, by index among NaNs
    odd = np.array([[np.nan, 0, 1, 1], [0, 0, np.inf, 1], [np.nan, 0, 1, 1], [.25, .25, .75, .75]], np.float32)
    assert AO.candidates(odd, [0, 4], np.array(box, np.float32), 3) == [0, 1, 3]
    assert AO.candidates(odd, [0, 4], np.array(box, np.float32), 2) == [1, 3]


def test_oracle_a_level_smaller_than_topk_is_taken_whole():
    priors = [[0, 0, .5, .5], [.5, .5, 1, 1], [0, .5, .5, 1], [.25, .25, .75, .75], [0, 0, 1, 1]]
    box = np.array([.25, .25, .75, .75], np.float32)
    assert AO.candidates(np.array(priors, np.float32), [0, 3, 4, 5], box, 2) == [0, 1, 3, 4]      # 2 of 3, 1 of 1, 1 of 1
    assert AO.candidates(np.array(priors, np.float32), [0, 3, 4, 5], box, 7) == [0, 1, 2, 3, 4]


def test_oracle_a_matched_prior_keeps_its_box_but_enters_the_statistic():
    priors = [[.25, .25, .75, .75], [0, 0, .5, .5], [.5, .5, 1, 1]]
    box = [.25, .25, .75, .75]
    free = _one(priors, [0, 3], [[0, 0, .125, .125], box], 3)
    held = _one(priors, [0, 3], [[0, 0, .125, .125], box], 3, match=[0, -1, -1])
    a = 0.0625 / (0.25 + 0.25 - 0.0625)                        # the IoUs are 1, a, a
    mean = ((1.0 + a) + a) / 3.0
    want_thr = mean + np.sqrt((((1.0 - mean) * (1.0 - mean) + (a - mean) * (a - mean)) + (a - mean) * (a - mean)) / 2.0)
    assert a < want_thr < 1.0
    assert free[0] == [1, -1, -1] and free[1] == 1 and free[2][1] == want_thr
    assert held[0] == [0, -1, -1] and held[1] == 0 and held[2] == free[2]      # the same thresholds, nothing reassigned


def test_oracle_skips_and_padding():
    c = AC.make_case("p70")
    full, full_extra, full_thr = AC.oracle("p70")
    st = np.array([0, 1, 2, 0], np.int32)
    out, extra, thr = AO.atss(c["priors"], c["levels"], c["gt"], c["n"], st, c["match"], c["topk"])
    assert np.array_equal(out[[0, 1, 2]], c["match"][[0, 1, 2]]) and extra[:3].tolist() == [0, 0, 0] and not thr[:3].any()
    assert np.array_equal(out[3], full[3]) and extra[3] == full_extra[3] and np.array_equal(thr[3], full_thr[3])
    nan_pad = c["gt"].copy()
    for b in range(c["B"]):
        nan_pad[b, c["n"][b]:] = np.nan
    again = AO.atss(c["priors"], c["levels"], nan_pad, c["n"], c["status"], c["match"], c["topk"])
    assert all(np.array_equal(x, y) for x, y in zip(again, (full, full_extra, full_thr)))


# ------------------------------------------------------------------------------------------------- the oracle, on the cases
def _survey(c):
    """What the case exercises: (second claims, candidates over their threshold with the centre outside the box, levels
    with bit-equal distances on both sides of the top-k cut)."""
    second = outside = ties = 0
    for b in range(c["B"]):
        claims = {}
        for j in range(c["n"][b]):
            cand, ious, thr, pos = AO.positives(c["priors"], c["levels"], c["gt"][b, j], c["topk"])
            with np.errstate(invalid="ignore"):
                outside += int(((ious > 0) & (ious >= thr) & ~pos).sum())
            for p in np.array(cand)[pos]:
                if c["match"][b, p] < 0:
                    claims[p] = claims.get(p, 0) + 1
            d2 = AO.distances(c["priors"], c["gt"][b, j])
            for lo, hi in zip(c["levels"][:-1], c["levels"][1:]):
                if c["topk"] < hi - lo:
                    s = np.sort(d2[lo:hi])
                    ties += int(s[c["topk"] - 1] == s[c["topk"]])
        second += sum(v - 1 for v in claims.values())
    return second, outside, ties


# Which case carries which condition.  Every case adds priors; second claims and positives lost to the centre rule need
# boxes that crowd each other, which the cases with 2 to 5 boxes among 70 random priors do not have.
CARRIES = {"p13": (True, False, False), "p70": (False, False, False), "p70_lattice": (False, False, True),
           "p646": (True, True, True), "p3199": (True, True, True), "p70_top1": (False, False, False),
           "p70_all": (True, True, False), "p646_deep": (True, True, False)}


@pytest.mark.parametrize("name", list(AC.CASES))
def test_oracle_properties_on_the_gpu_cases(name):
    c = AC.make_case(name)
    out, n_extra, thr = AC.oracle(name)
    second, outside, ties = _survey(c)
    print(name, "boxes", c["n"].tolist(), "added", n_extra.tolist(), "second claims", second, "over the threshold but outside",
          outside, "levels with equal distances across the cut", ties)
    assert n_extra.sum() > 0 and n_extra[0] == 0 and c["n"][0] == 0
    for got, wanted in zip((second, outside, ties), CARRIES[name]):
        assert not wanted or got > 0
    had = c["match"] >= 0
    assert np.array_equal(out[had], c["match"][had])                           # a matched prior is never reassigned
    assert np.array_equal(n_extra, ((out >= 0) & ~had).sum(1))
    for b in range(c["B"]):
        assert not thr[b, c["n"][b]:].any() and (out[b] < c["n"][b]).all()
        for j in range(c["n"][b]):
            cand, ious, t, pos = AO.positives(c["priors"], c["levels"], c["gt"][b, j], c["topk"])
            assert len(cand) == sum(min(c["topk"], hi - lo) for lo, hi in zip(c["levels"][:-1], c["levels"][1:]))
            assert cand == sorted(set(cand)) and t == thr[b, j]
            for p in np.nonzero((out[b] == j) & ~had[b])[0]:                   # every added prior is a positive of its box
                assert pos[cand.index(p)]
