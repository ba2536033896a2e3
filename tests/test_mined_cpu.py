"""Hard-negative mining of the confidence loss, the parts that need no GPU: the config keys, the numpy restatement the
GPU tests compare against (tests/mined_oracle.py), and the ctypes table."""
import numpy as np
import pytest

from tests import mined_oracle as MO
from oracle import ref_numpy as R


# ------------------------------------------------------------------------------------------------- config keys
@pytest.mark.parametrize("cfg,want", [
    ({}, None),
    ({"LOSS_NEG_PER_POS": None}, None),
    ({"LOSS_NEG_PER_POS": None, "LOSS_MIN_NEG": None}, None),
    ({"LOSS_NEG_PER_POS": 3}, (3, 0)),
    ({"LOSS_NEG_PER_POS": 1, "LOSS_MIN_NEG": 0}, (1, 0)),
    ({"LOSS_NEG_PER_POS": 3, "LOSS_MIN_NEG": 5}, (3, 5)),
    ({"LOSS_NEG_PER_POS": 3.0, "LOSS_MIN_NEG": 5.0}, (3, 5)),
    ({"LOSS_NEG_PER_POS": 3, "LOSS_MIN_NEG": None}, (3, 0)),
])
def test_negative_mining_accepts(cfg, want):
    from multibox_amd.config import Cfg, negative_mining, with_defaults
    assert negative_mining(Cfg(cfg)) == want
    got = negative_mining(with_defaults(Cfg(cfg)))            # the defaults switch nothing on
    assert got == want and (got is None or all(type(v) is int for v in got))


@pytest.mark.parametrize("cfg,key", [
    ({"LOSS_NEG_PER_POS": 0}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": -2}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": True}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": 2.5}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": "3"}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": float("nan")}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": 2 ** 31}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": [3]}, "LOSS_NEG_PER_POS"),
    ({"LOSS_NEG_PER_POS": 3, "LOSS_MIN_NEG": -1}, "LOSS_MIN_NEG"),
    ({"LOSS_NEG_PER_POS": 3, "LOSS_MIN_NEG": False}, "LOSS_MIN_NEG"),
    ({"LOSS_NEG_PER_POS": 3, "LOSS_MIN_NEG": 0.5}, "LOSS_MIN_NEG"),
    ({"LOSS_NEG_PER_POS": 3, "LOSS_MIN_NEG": "5"}, "LOSS_MIN_NEG"),
    ({"LOSS_MIN_NEG": 5}, "LOSS_MIN_NEG"),
    ({"LOSS_NEG_PER_POS": None, "LOSS_MIN_NEG": 0}, "LOSS_MIN_NEG"),
])
def test_negative_mining_rejects(cfg, key):
    from multibox_amd.config import Cfg, negative_mining
    with pytest.raises(ValueError, match=key):
        negative_mining(Cfg(cfg))


def test_train_py_names_the_bad_key_before_it_touches_the_gpu(tmp_path, monkeypatch):
    import torch
    import train
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE: 2\nLOSS_NEG_PER_POS: 2.5\n")

    def no_gpu(*a, **k):
        raise AssertionError("torch.cuda.set_device was reached")
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    monkeypatch.setattr("sys.argv", ["train.py", "--priors", str(tmp_path / "priors.pkl"), "--logdir", str(tmp_path),
                                     "--config", str(cfg), "--synthetic"])
    with pytest.raises(SystemExit, match="LOSS_NEG_PER_POS"):
        train.main()


# ------------------------------------------------------------------------------------------------- the oracle
def _case(seed, B, P, G, quantised=False):
    rng = np.random.RandomState(seed)
    conf = rng.uniform(0.01, 0.99, (B, P)).astype(np.float32)
    if quantised:
        conf = (np.floor(conf * 16) / 16).astype(np.float32)
    match = -np.ones((B, P), np.int32)
    n_pos = rng.randint(0, min(G, P) + 1, B)
    n_pos[0], n_pos[-1] = 0, min(G, P)
    for b in range(B):
        match[b, rng.permutation(P)[:n_pos[b]]] = rng.permutation(G)[:n_pos[b]]
    return conf, match, n_pos


def test_score_order_key_orders_like_the_floats():
    x = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 0.25, 1.0, np.inf, np.nan], np.float32)
    k = MO.score_order_key(x).astype(np.int64)
    assert k[3] == k[4] == 0x80000000                         # -0 == +0
    assert np.all(np.diff(np.delete(k, 3)) > 0)               # strictly increasing otherwise, the NaN on top
    assert k[-1] == 0xffffffff and MO.score_order_key(np.array([-np.nan], np.float32))[0] == 0xffffffff


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("B,P,G,neg_per_pos,min_neg", [(3, 13, 13, 3, 0), (4, 70, 5, 3, 0), (4, 646, 13, 3, 5),
                                                        (3, 3199, 100, 50, 0), (2, 646, 13, 2 ** 31 - 1, 0)])
def test_oracle_mask_is_the_top_k_of_the_negatives(B, P, G, neg_per_pos, min_neg, quantised):
    conf, match, n_pos = _case(P, B, P, G, quantised)
    mask, K = MO.select(conf, match, neg_per_pos, min_neg)
    key = MO.score_order_key(conf).astype(np.int64)
    for b in range(B):
        n_negatives = P - n_pos[b]
        assert K[b] == min(n_negatives, max(min_neg, neg_per_pos * int(n_pos[b])))
        assert mask[b].sum() == K[b] and not mask[b][match[b] >= 0].any()
        sel, rest = np.nonzero(mask[b])[0], np.nonzero((match[b] < 0) & ~mask[b])[0]
        if len(sel) and len(rest):
            # every unselected negative ranks after every selected one: (key descending, index ascending)
            worst = max(sel, key=lambda p: (-key[b, p], p))
            best = min(rest, key=lambda p: (-key[b, p], p))
            assert (-key[b, worst], worst) < (-key[b, best], best)
    assert K[0] == min(P, min_neg)                            # an image without positives keeps min_neg


def test_oracle_breaks_ties_by_index_and_takes_a_nan_first():
    conf = np.array([[0.5, 0.25, 0.5, -0.0, 0.5, 0.0, np.nan, 0.5]], np.float32)
    match = np.array([[-1, 0, -1, -1, -1, -1, -1, -1]], np.int32)
    for k, want in [(1, [6]), (3, [6, 0, 2]), (5, [6, 0, 2, 4, 7]), (6, [6, 0, 2, 4, 7, 3]), (7, [6, 0, 2, 4, 7, 3, 5])]:
        mask, K = MO.select(conf, match, k, 0)
        assert K[0] == k and sorted(np.nonzero(mask[0])[0]) == sorted(want)


@pytest.mark.parametrize("conf_is_logit", [1, 0])
def test_all_negatives_selected_is_ref_numpy_exactly(conf_is_logit):
    B, P, G = 3, 70, 5
    conf, match, n_pos = _case(7, B, P, G)
    rng = np.random.RandomState(8)
    dec = rng.uniform(0, 1, (B, P, 4)).astype(np.float32)
    gt = rng.uniform(0, 1, (B, G, 4)).astype(np.float32)
    x = (rng.randn(B, P) * 2 - 1).astype(np.float32) if conf_is_logit else conf
    out = MO.mined_loss(dec, x, conf_is_logit, gt, match, 1000.0, 3, P)
    assert np.array_equal(out["n_neg"], P - n_pos) and np.array_equal(out["mask"], match < 0)
    zero = np.zeros((P, 4), np.float32)
    ref = R.add_loss(dec, R.sigmoid_f32(x) if conf_is_logit else x, gt, n_pos, zero, 1000.0, match=match)
    assert out["loc_loss"].tobytes() == ref["loc_loss"].tobytes() and out["conf_loss"].tobytes() == ref["conf_loss"].tobytes()
    if conf_is_logit:
        dl, dz = R.add_loss_grads(dec, x, gt, zero, 1000.0, match)
        assert out["d_locs"].tobytes() == dl.tobytes() and out["d_conf_in"].tobytes() == dz.tobytes()
    # and with fewer: the dropped negatives' terms are gone, nothing else moves
    few = MO.mined_loss(dec, x, conf_is_logit, gt, match, 1000.0, 3, 0)
    dropped = (match < 0) & ~few["mask"]
    assert dropped.any() and np.all(few["d_conf_in"][dropped] == 0)
    assert np.array_equal(few["d_conf_in"][~dropped], out["d_conf_in"][~dropped])
    assert few["loc_loss"] == out["loc_loss"] and few["conf_loss"] < out["conf_loss"]
    c = ((R.sigmoid_f32(x) if conf_is_logit else x) + np.float32(1e-10)).astype(np.float32)
    u = ((np.float32(1) - c) + np.float32(1e-10)).astype(np.float32)
    gone = -np.log(u[dropped]).astype(np.float64).sum()
    assert np.isclose(float(out["conf_loss"]) - float(few["conf_loss"]), gone, rtol=1e-5)


# ------------------------------------------------------------------------------------------------- ctypes table
def test_ctypes_table_declares_the_mined_entry_points():
    import ctypes as C
    from multibox_amd import _lib
    assert {"mbx_loss_mined_workspace_bytes", "mbx_loss_fwd_bwd_mined"} <= set(_lib.declared_symbols())
    res, args = _lib._SIGS["mbx_loss_fwd_bwd_mined"]
    plain = _lib._SIGS["mbx_loss_fwd_bwd"][1]
    # every argument of mbx_loss_fwd_bwd in its order, then neg_per_pos, min_neg, n_neg in front of the workspace
    assert res is C.c_int and args == plain[:13] + [C.c_int, C.c_int, C.c_void_p] + plain[13:]
    assert _lib._SIGS["mbx_loss_mined_workspace_bytes"] == (C.c_size_t, [C.c_int, C.c_int])
