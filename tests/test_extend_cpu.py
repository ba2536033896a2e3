"""Threshold matching (mbx_match_extend), the parts that need no GPU: the config key, the numpy restatement the GPU tests
compare against (tests/extend_oracle.py), and the ctypes table."""
import re
import os

import numpy as np
import pytest

from tests import extend_oracle as EO

KEY = "LOSS_MATCH_IOU_THRESHOLD"


# ------------------------------------------------------------------------------------------------- config key
@pytest.mark.parametrize("cfg,want", [
    ({}, None),
    ({KEY: None}, None),
    ({KEY: 0.5}, 0.5),
    ({KEY: 1}, 1.0),
    ({KEY: 1.0}, 1.0),
    ({KEY: 1e-3}, 1e-3),
])
def test_match_iou_threshold_accepts(cfg, want):
    from multibox_amd.config import Cfg, match_iou_threshold, with_defaults
    assert match_iou_threshold(Cfg(cfg)) == want
    got = match_iou_threshold(with_defaults(Cfg(cfg)))        # the defaults switch nothing on
    assert got == want and (got is None or type(got) is float)


@pytest.mark.parametrize("value", [0, 0.0, -0.1, 1.5, 2, True, False, "0.5", [0.5], float("nan"), float("inf")])
def test_match_iou_threshold_rejects(value):
    from multibox_amd.config import Cfg, match_iou_threshold
    with pytest.raises(ValueError, match=KEY):
        match_iou_threshold(Cfg({KEY: value}))


def test_the_mining_keys_and_this_one_do_not_see_each_other():
    from multibox_amd.config import Cfg, match_iou_threshold, negative_mining
    cfg = Cfg({KEY: 0.4, "LOSS_NEG_PER_POS": 3})
    assert match_iou_threshold(cfg) == 0.4 and negative_mining(cfg) == (3, 0)
    assert negative_mining(Cfg({KEY: 0.4})) is None and match_iou_threshold(Cfg({"LOSS_NEG_PER_POS": 3})) is None


def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch):
    import torch
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\n%s: 1.5\n" % KEY)

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match=KEY):
        train.main()


def test_multibox_loss_keyword_allocates_n_extra_and_refuses_a_bad_value():
    import torch
    import __graft_entry__ as g
    g.build()                                                 # the constructor asks the library for its workspace size
    from multibox_amd import loss as L
    priors = np.array([[0, 0, .5, .5], [.25, .25, 1, 1]], np.float32)
    assert L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu").n_extra is None
    ml = L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", match_iou_threshold=0.5)
    assert ml.n_extra.dtype == torch.int32 and ml.n_extra.shape == (3,) and ml.match_iou_threshold == 0.5
    for bad in (0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="match_iou_threshold"):
            L.MultiboxLoss(priors, 3, 13, 1000.0, device="cpu", match_iou_threshold=bad)


# ------------------------------------------------------------------------------------------------- the oracle
def _case(seed, B, P, G, grid=None):
    """Priors on a jittered lattice, boxes that are jittered copies of random priors, a random subset of the priors
    already matched to distinct boxes.  Image 0 has no box."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(0.1, 0.9, (P, 2)); wh = rng.uniform(0.05, 0.4, (P, 2))
    priors = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    n = rng.randint(1, min(G, P) + 1, B)
    n[0] = 0
    gt = np.zeros((B, G, 4), np.float32)
    match = -np.ones((B, P), np.int32)
    for b in range(B):
        src = priors[rng.randint(0, P, n[b])]
        gt[b, :n[b]] = src + rng.uniform(-0.02, 0.02, (n[b], 4)).astype(np.float32)
        match[b, rng.permutation(P)[:n[b]]] = rng.permutation(n[b])
    if grid:
        priors = (np.round(priors * grid) / grid).astype(np.float32)
        gt = (np.round(gt * grid) / grid).astype(np.float32)
    return priors, gt, n.astype(np.int32), np.zeros(B, np.int32), match


def test_iou_row_known_values():
    iou = EO.iou_row([0, 0, .5, .5], [[0, 0, .5, .25], [.5, .5, 1, 1], [.25, .25, .75, .75], [0, 0, .5, .5], [.2, .2, .2, .9]])
    assert iou.tolist() == [0.5, 0.0, 0.0625 / 0.4375, 1.0, 0.0]


@pytest.mark.parametrize("thr", [0.3, 0.5])
@pytest.mark.parametrize("B,P,G", [(3, 13, 13), (4, 70, 5), (3, 646, 13)])
def test_oracle_properties(B, P, G, thr):
    priors, gt, n, status, match = _case(P, B, P, G)
    out, n_extra = EO.extend(priors, gt, n, status, match, thr)
    assert n_extra.sum() > 0 and n_extra[0] == 0
    assert np.array_equal(out[match >= 0], match[match >= 0])                 # a matched prior is never reassigned
    assert np.array_equal(n_extra, ((out >= 0) & (match < 0)).sum(1))
    for b in range(B):
        for p in np.nonzero(match[b] < 0)[0]:
            iou = EO.iou_row(priors[p], gt[b, :n[b]]) if n[b] else np.zeros(1)
            if out[b, p] >= 0:
                j = out[b, p]
                assert j < n[b] and iou[j] > float(np.float32(thr)) and iou[j] == iou.max()
                assert not (iou[:j] == iou[j]).any()                          # the lowest index among equals
            else:
                assert not (iou > float(np.float32(thr))).any()


def test_oracle_ties_go_to_the_lowest_index():
    priors = np.array([[.25, .25, .75, .75]], np.float32)
    box = [.25, .25, .75, .5]                                                 # IoU exactly 0.5 with the prior
    gt = np.array([[[0, 0, .1, .1], box, box, [.25, .25, .75, .75]]], np.float32)
    free = -np.ones((1, 1), np.int32)
    out, n_extra = EO.extend(priors, gt, [3], [0], free, 0.4)
    assert out.tolist() == [[1]] and n_extra.tolist() == [1]                  # 1 and 2 are equal: 1
    out, _ = EO.extend(priors, gt, [4], [0], free, 0.4)
    assert out.tolist() == [[3]]                                              # a larger IoU later wins
    out, n_extra = EO.extend(priors, gt, [3], [0], free, 0.5)
    assert out.tolist() == [[-1]] and n_extra.tolist() == [0]                 # strict: 0.5 is not over 0.5
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert EO.extend(priors, gt, [3], [0], free, below)[0].tolist() == [[1]]


def test_oracle_skips_and_threshold_one():
    priors, gt, n, status, match = _case(5, 4, 70, 5)
    out, n_extra = EO.extend(priors, gt, n, status, match, 1.0)
    assert np.array_equal(out, match) and not n_extra.any()                   # no IoU exceeds 1
    gt1 = gt.copy()
    gt1[1, 0] = priors[np.nonzero(match[1] < 0)[0][0]]                        # an IoU of exactly 1 is still not over 1
    out, n_extra = EO.extend(priors, gt1, n, status, match, 1.0)
    assert np.array_equal(out, match) and not n_extra.any()
    st = np.array([0, 1, 2, 0], np.int32)
    out, n_extra = EO.extend(priors, gt, n, st, match, 0.3)
    full, full_extra = EO.extend(priors, gt, n, status, match, 0.3)
    assert np.array_equal(out[[1, 2]], match[[1, 2]]) and n_extra[[1, 2]].tolist() == [0, 0]
    assert np.array_equal(out[3], full[3]) and full_extra[1:].min() > 0
    nan_pad = gt.copy()
    for b in range(4):
        nan_pad[b, n[b]:] = np.nan                                            # padding rows are never read
    assert np.array_equal(EO.extend(priors, nan_pad, n, status, match, 0.3)[0], full)


# ------------------------------------------------------------------------------------------------- ctypes table
def test_ctypes_signature_has_the_argument_order_of_the_header():
    import ctypes as C
    from multibox_amd import _lib
    assert "mbx_match_extend" in _lib.declared_symbols()
    res, args = _lib._SIGS["mbx_match_extend"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mbx.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+mbx_match_extend\s*\(([^)]*)\)", hdr)
    assert m, "include/mbx.h does not declare mbx_match_extend"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["priors", "gt", "n_gt", "status", "iou_threshold", "B", "P", "G",
                                                           "match", "n_extra", "stream"]
    kind = lambda p: C.c_void_p if "*" in p or p.startswith("mbx_stream_t") else {"float": C.c_float, "int": C.c_int}[p.split()[0]]
    assert res is C.c_int and args == [kind(p) for p in params]
