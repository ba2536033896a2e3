"""GPU: mbx_loss_fwd_bwd_focal (the focal loss on the confidence term, with or without hard-negative mining) against
tests/focal_oracle.py.

The C ABI is driven directly with a hand-made `match`, so nothing before the MultiboxLoss tests depends on the matcher.
Bars, the project's own for this loss (test_gpu_postproc.py, test_gpu_loss_mined.py): the selection (which negatives
count, n_neg, the +0 gradients of the others) is exact; loss values rtol 1e-5, gradients rtol 1e-4 / atol 1e-6;
gamma = 0 with unit weights is byte-identical to mbx_loss_fwd_bwd / mbx_loss_fwd_bwd_mined.
"""
import numpy as np
import pytest

from tests import focal_oracle as FO
from tests import mined_oracle as MO
from tests.loss_cases import (ALPHA, SENTINEL, SHAPES, _forward_backward, batch, call, cut_splits_a_run, gpu, make_case,  # noqa: F401
                              weights)

pytestmark = pytest.mark.gpu

FOCAL = [(2.0, 0.25), (0.5, None), (5.0, 0.75)]              # (gamma, alpha); alpha None = weights (1, 1)


def oracle(c, conf_in, is_logit, gamma, alpha, neg_per_pos=0, min_neg=0, w=None):
    w_pos, w_neg = weights(alpha) if w is None else w
    return FO.focal_loss(c["dec"], conf_in, is_logit, c["gt"], c["match"], ALPHA, gamma, w_pos, w_neg, neg_per_pos, min_neg)


def check_values(out, ref, what=""):
    """The bars of the module docstring; every figure is printed before it is asserted."""
    err = np.abs(out["dz"].astype(np.float64) - ref["d_conf_in"]) / (1e-6 + 1e-4 * np.abs(ref["d_conf_in"]))
    rel = abs(float(out["loss2"][1]) - float(ref["conf_loss"])) / max(abs(float(ref["conf_loss"])), 1e-30)
    print("%s conf_loss %r oracle %r rel %.3g; worst gradient error %.3g x bar" % (
        what, out["loss2"][1], ref["conf_loss"], rel, err.max()))
    assert np.array_equal(out["n_neg"], ref["n_neg"])
    assert np.isfinite(out["loss2"]).all() and np.isfinite(out["dz"]).all() and np.isfinite(out["dl"]).all()
    assert np.isclose(out["loss2"][0], ref["loc_loss"], rtol=1e-5) and np.isclose(out["loss2"][1], ref["conf_loss"], rtol=1e-5)
    assert np.allclose(out["dl"], ref["d_locs"], rtol=1e-4, atol=1e-6)
    assert np.allclose(out["dz"], ref["d_conf_in"], rtol=1e-4, atol=1e-6)


def same_bytes(a, b, keys=("loss2", "dl", "dz", "n_neg")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


# --------------------------------------------------------------------------------------------- 1. values, 4. location
@pytest.fixture(scope="module")
def plain_results(gpu):
    """mbx_loss_fwd_bwd on every shape and both input kinds, computed once."""
    out = {}
    for B, P, G in SHAPES:
        c = make_case(B, P, G)
        for is_logit in (1, 0):
            st, out[(B, P, G, is_logit)] = call(gpu, c, c["z"] if is_logit else c["x"], is_logit, entry="plain")
            assert st == 0
    return out


@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
@pytest.mark.parametrize("gamma,alpha", FOCAL)
@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_values_against_the_oracle_and_location_untouched(gpu, plain_results, B, P, G, is_logit, gamma, alpha, neg_per_pos):
    c = make_case(B, P, G)
    x = c["z"] if is_logit else c["x"]
    ref = oracle(c, x, is_logit, gamma, alpha, neg_per_pos)
    st, out = call(gpu, c, x, is_logit, gamma=gamma, alpha=alpha, neg_per_pos=neg_per_pos)
    assert st == 0
    check_values(out, ref, "P=%d logit=%d gamma=%g alpha=%r neg_per_pos=%d:" % (P, is_logit, gamma, alpha, neg_per_pos))
    if neg_per_pos == 0:
        assert np.array_equal(out["n_neg"], P - c["n_pos"])
    dropped = (c["match"] < 0) & ~ref["mask"]
    assert np.all(out["dz"].view(np.uint32)[dropped] == 0)
    # the location loss and its gradient are mbx_loss_fwd_bwd's, byte for byte
    plain = plain_results[(B, P, G, is_logit)]
    assert out["dl"].tobytes() == plain["dl"].tobytes() and out["loss2"][:1].tobytes() == plain["loss2"][:1].tobytes()


# ------------------------------------------------------------------------------- 2. gamma = 0, weights (1, 1): the old bytes
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
def test_gamma_zero_unit_weights_is_the_unmined_entry_byte_for_byte(gpu, B, P, G, is_logit):
    c = make_case(B, P, G)
    x = c["z"] if is_logit else c["x"]
    st_f, focal = call(gpu, c, x, is_logit, gamma=0.0, alpha=None, grad_scale=0.25)
    st_p, plain = call(gpu, c, x, is_logit, entry="plain", grad_scale=0.25)
    assert st_f == 0 and st_p == 0
    same_bytes(focal, plain, ("loss2", "dl", "dz"))
    assert np.array_equal(focal["n_neg"], P - c["n_pos"])


@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit,kind,min_neg", [(1, "plain", 0), (0, "plain", 0), (1, "plain", None), (0, "quantised", 0),
                                                   (0, "quantised", 5)])
def test_gamma_zero_unit_weights_is_the_mined_entry_byte_for_byte(gpu, B, P, G, is_logit, kind, min_neg):
    c = make_case(B, P, G, kind)
    x = c["z"] if is_logit else c["x"]
    min_neg = P if min_neg is None else min_neg
    st_f, focal = call(gpu, c, x, is_logit, gamma=0.0, alpha=None, neg_per_pos=3, min_neg=min_neg, grad_scale=0.25)
    st_m, mined = call(gpu, c, x, is_logit, entry="mined", neg_per_pos=3, min_neg=min_neg, grad_scale=0.25)
    assert st_f == 0 and st_m == 0
    same_bytes(focal, mined)
    assert np.array_equal(focal["n_neg"], MO.n_selected(c["match"], 3, min_neg))


# --------------------------------------------------------------------------------------- 3. the weights, without the oracle
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
def test_gamma_zero_alpha_half_halves_every_gradient_exactly(gpu, B, P, G, is_logit):
    c = make_case(B, P, G)
    x = c["z"] if is_logit else c["x"]
    st_f, focal = call(gpu, c, x, is_logit, gamma=0.0, alpha=0.5)
    st_p, plain = call(gpu, c, x, is_logit, entry="plain")
    assert st_f == 0 and st_p == 0
    assert focal["dz"].tobytes() == (np.float32(0.5) * plain["dz"]).tobytes()
    print("conf_loss", focal["loss2"][1], "half the plain one", 0.5 * float(plain["loss2"][1]))
    assert np.isclose(focal["loss2"][1], 0.5 * float(plain["loss2"][1]), rtol=1e-5)
    assert focal["dl"].tobytes() == plain["dl"].tobytes() and focal["loss2"][:1].tobytes() == plain["loss2"][:1].tobytes()


# ---------------------------------------------------------------------------------------------- 5. selection under mining
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("kind,min_neg", [("plain", 0), ("plain", 5), ("quantised", 0), ("zeros", None)])
def test_selection_under_mining_is_the_mined_entrys(gpu, B, P, G, kind, min_neg):
    c = make_case(B, P, G, kind)
    min_neg = P // 2 if min_neg is None else min_neg          # zeros: the cut has to reach the run of zeros
    mask, K = MO.select(c["x"], c["match"], 3, min_neg)
    st, out = call(gpu, c, c["x"], 0, gamma=2.0, alpha=0.25, neg_per_pos=3, min_neg=min_neg)
    assert st == 0
    neg = c["match"] < 0
    assert np.array_equal(out["n_neg"], K)
    # a selected negative's gradient w_neg (c^2 / w - 2 c log w) is > 0 in float32 even at c = 1e-10 (1e-20 / 1)
    assert np.array_equal((out["dz"] != 0) & neg, mask)
    assert np.all(out["dz"].view(np.uint32)[neg & ~mask] == 0)            # +0.0f by bits
    assert np.all(out["dz"][~neg] < 0)
    if kind in ("quantised", "zeros") and P >= 70:
        assert cut_splits_a_run(c, mask)                      # the cut falls inside a run of equal keys


# ------------------------------------------------------------------------------------------------------- 6. saturation
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0, 10.0])
@pytest.mark.parametrize("is_logit", [1, 0])
def test_saturated_inputs_stay_finite_and_within_the_bars(gpu, gamma, is_logit):
    c = make_case(4, 70, 5)
    rng = np.random.RandomState(11)
    sat = np.array([30, -30, 100, -100], np.float32) if is_logit else np.array([0.0, 1.0], np.float32)
    x = (c["z"] if is_logit else c["x"]).copy()
    hit = rng.uniform(size=x.shape) < 0.5
    x[hit] = sat[rng.randint(0, len(sat), int(hit.sum()))]
    for b in range(4):                                        # every saturated value on a positive and on a negative
        pos, neg = np.nonzero(c["match"][b] >= 0)[0], np.nonzero(c["match"][b] < 0)[0]
        if len(pos) >= len(sat):
            x[b, pos[:len(sat)]] = sat
        x[b, neg[:len(sat)]] = sat
    s, _, _ = FO.scw(x, is_logit)
    assert (s == 0).any() and (s == 1).any()                  # s is exactly 0 and exactly 1 somewhere
    for alpha, neg_per_pos in ((None, 0), (0.25, 0), (0.25, 3)):
        ref = oracle(c, x, is_logit, gamma, alpha, neg_per_pos)
        assert np.isfinite(ref["d_conf_in"]).all() and np.isfinite(ref["conf_loss"])
        st, out = call(gpu, c, x, is_logit, gamma=gamma, alpha=alpha, neg_per_pos=neg_per_pos)
        assert st == 0
        check_values(out, ref, "saturated logit=%d gamma=%g alpha=%r neg_per_pos=%d:" % (is_logit, gamma, alpha, neg_per_pos))


# ------------------------------------------------------------------------------------------------------- 7. grad_scale
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
def test_grad_scale_scales_the_kept_gradients_exactly(gpu, B, P, G, is_logit):
    c = make_case(B, P, G)
    x = c["z"] if is_logit else c["x"]
    mask, _ = MO.select(x, c["match"], 3, 0)
    dropped = (c["match"] < 0) & ~mask
    st_a, one = call(gpu, c, x, is_logit, gamma=2.0, alpha=0.25, neg_per_pos=3)
    st_b, neg = call(gpu, c, x, is_logit, gamma=2.0, alpha=0.25, neg_per_pos=3, grad_scale=-0.5)
    assert st_a == 0 and st_b == 0
    assert neg["loss2"].tobytes() == one["loss2"].tobytes()
    assert np.array_equal(neg["dz"][~dropped], one["dz"][~dropped] * np.float32(-0.5))
    assert np.array_equal(neg["dl"], one["dl"] * np.float32(-0.5))
    assert np.all(neg["dz"].view(np.uint32)[dropped] == 0)


# ------------------------------------------------------------------------------------- 8. independence and repeatability
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, B, P, G, neg_per_pos):
    c = make_case(B, P, G, "quantised")
    _, full = call(gpu, c, c["x"], 0, neg_per_pos=neg_per_pos)
    _, again = call(gpu, c, c["x"], 0, neg_per_pos=neg_per_pos)
    same_bytes(full, again)
    for b in range(B):
        st, alone = call(gpu, c, c["x"], 0, neg_per_pos=neg_per_pos, rows=slice(b, b + 1))
        assert st == 0
        assert alone["dz"].tobytes() == full["dz"][b:b + 1].tobytes() and alone["n_neg"][0] == full["n_neg"][b]
        assert alone["dl"].tobytes() == full["dl"][b:b + 1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 9. NaN
def test_a_nan_negative_is_taken_first_and_only_where_something_is_taken(gpu):
    c = make_case(4, 70, 5)
    neg1, neg0 = np.nonzero(c["match"][1] < 0)[0], np.nonzero(c["match"][0] < 0)[0]
    z = c["z"].copy()
    z[1, neg1[-1]] = np.nan                                   # image 1: 5 positives, K = 15
    mask, K = MO.select(z, c["match"], 3, 0)
    assert K[1] == 15 and mask[1, neg1[-1]]
    st, out = call(gpu, c, z, 1, neg_per_pos=3)
    assert st == 0 and np.array_equal(out["n_neg"], K)
    assert np.isnan(out["dz"][1, neg1[-1]]) and np.isnan(out["loss2"][1]) and np.isfinite(out["loss2"][0])
    assert np.array_equal((out["dz"] != 0) & (c["match"] < 0), mask)
    z = c["z"].copy()
    z[0, neg0[3]] = np.nan                                    # image 0: no positive, K = 0: the NaN is never looked at
    st, out = call(gpu, c, z, 1, neg_per_pos=3)
    assert st == 0 and out["n_neg"][0] == 0
    assert np.isfinite(out["loss2"]).all() and not out["dz"][0].any()


# ------------------------------------------------------------------------------------------------------------ 10. errors
@pytest.mark.parametrize("kw,status", [
    (dict(gamma=-0.5), -1), (dict(gamma=10.5), -1), (dict(gamma=float("nan")), -1), (dict(gamma=float("inf")), -1),
    (dict(w=(-0.25, 1.0)), -1), (dict(w=(1.0, -0.25)), -1), (dict(w=(float("inf"), 1.0)), -1),
    (dict(w=(1.0, float("inf"))), -1), (dict(w=(float("nan"), 1.0)), -1), (dict(w=(1.0, float("nan"))), -1),
    (dict(neg_per_pos=-1), -1), (dict(neg_per_pos=3, min_neg=-1), -1), (dict(neg_per_pos=0, min_neg=1), -1),
    (dict(ws_short=1), -4), (dict(neg_per_pos=3, ws_short=1), -4)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, kw, status):
    c = make_case(4, 70, 5)
    st, out = call(gpu, c, c["z"], 1, prefill=SENTINEL, **kw)
    assert st == status
    assert np.all(out["loss2"] == SENTINEL) and np.all(out["dl"] == SENTINEL) and np.all(out["dz"] == SENTINEL)
    assert np.all(out["n_neg"] == int(SENTINEL))
    st, out = call(gpu, c, c["z"], 1, prefill=SENTINEL)       # the same buffers are written by a good call
    assert st == 0 and not np.any(out["dz"] == SENTINEL) and not np.any(out["n_neg"] == int(SENTINEL))
    assert not np.any(out["loss2"] == SENTINEL) and not np.any(out["dl"] == SENTINEL)


def test_what_the_plain_entry_rejects_is_rejected(gpu):
    torch, l = gpu
    c = make_case(4, 70, 5)
    t = {k: torch.from_numpy(c[k]).cuda() for k in ("dec", "z", "gt", "match")}
    loss2 = torch.full((2,), SENTINEL, device="cuda")
    ws = torch.empty((l.mbx_loss_focal_workspace_bytes(4, 70),), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def go(dec=t["dec"].data_ptr(), z=t["z"].data_ptr(), gt=t["gt"].data_ptr(), match=t["match"].data_ptr(),
           out=loss2.data_ptr(), B=4, P=70, G=5, w=ws.data_ptr()):
        return l.mbx_loss_fwd_bwd_focal(dec, z, 1, gt, match, ALPHA, 1.0, B, P, G, out, None, None, 2.0, 0.25, 0.75, 0, 0,
                                        None, w, ws.numel(), s)
    for kw in (dict(dec=None), dict(z=None), dict(gt=None), dict(match=None), dict(out=None), dict(B=0), dict(B=-1),
               dict(P=0), dict(G=0)):
        assert go(**kw) == -1, kw
    assert go(w=None) == -4
    torch.cuda.synchronize()
    assert np.all(loss2.cpu().numpy() == SENTINEL)
    assert go() == 0                                          # d_raw_locs, d_logits and n_neg may all be NULL
    torch.cuda.synchronize()
    ref = oracle(c, c["z"], 1, 2.0, 0.25)
    assert np.isclose(loss2.cpu().numpy()[1], ref["conf_loss"], rtol=1e-5)


# ------------------------------------------------------------------------------------------- 11. through MultiboxLoss
def test_multibox_loss_without_the_switch_is_unchanged(gpu, batch):
    torch, _ = gpu
    from multibox_amd import loss as L
    for kw in (dict(), dict(neg_per_pos=3, min_neg=2), dict(match_iou_threshold=0.3)):
        old = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, **kw)            # the call as it always was
        new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, focal_gamma=None, focal_alpha=None, **kw)
        assert new.focal is None and new.ws.numel() == old.ws.numel() and (new.n_neg is None) == (old.n_neg is None)
        a, b = _forward_backward(torch, old, batch), _forward_backward(torch, new, batch)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    # and without any switch both are mbx_loss_fwd_bwd on the matcher's output
    plain = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA)
    b = _forward_backward(torch, plain, batch)
    c = dict(dec=plain.decoded.cpu().numpy(), gt=batch["gt"], match=plain.match.cpu().numpy(), P=batch["P"], G=batch["G"])
    _, direct = call(gpu, c, batch["logits"], 1, entry="plain")
    assert direct["loss2"].tobytes() == b[0].tobytes() and direct["dz"].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("kw", [dict(focal_gamma=2.0, focal_alpha=0.25), dict(focal_gamma=0.5),
                                dict(focal_gamma=2.0, focal_alpha=0.25, neg_per_pos=3, min_neg=2),
                                dict(focal_gamma=2.0, focal_alpha=0.25, neg_per_pos=3, match_iou_threshold=0.3)])
def test_multibox_loss_focal_with_the_real_matcher(gpu, batch, kw):
    torch, _ = gpu
    from multibox_amd import loss as L
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, **kw)
    loss2, dl, dz = _forward_backward(torch, ml, batch)
    match = ml.match.cpu().numpy()
    n_matched = (match >= 0).sum(1)
    if "match_iou_threshold" in kw:
        n_extra = ml.n_extra.cpu().numpy()
        assert np.array_equal(n_matched, batch["n"] + n_extra) and n_extra.sum() > 0      # the extended match is what is read
    else:
        assert np.array_equal(n_matched, batch["n"])
    neg_per_pos, min_neg = kw.get("neg_per_pos", 0), kw.get("min_neg", 0)
    w_pos, w_neg = weights(kw.get("focal_alpha"))
    ref = FO.focal_loss(ml.decoded.cpu().numpy(), batch["logits"], 1, batch["gt"], match, ALPHA, kw["focal_gamma"], w_pos,
                        w_neg, neg_per_pos, min_neg)
    if neg_per_pos:
        assert np.array_equal(ml.n_neg.cpu().numpy(), ref["n_neg"]) and np.array_equal(ref["n_neg"], MO.n_selected(match, 3, min_neg))
        assert np.array_equal((dz != 0) & (match < 0), ref["mask"])
    else:
        assert ml.n_neg is None
    check_values(dict(loss2=loss2, dl=dl, dz=dz, n_neg=ref["n_neg"]), ref, "MultiboxLoss %r:" % (kw,))


# --------------------------------------------------------------------------------------------- 12. through the Trainer
def test_trainer_step_focal_graph_equals_eager(gpu):
    torch, _ = gpu
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer
    from multibox_amd import priors as PR
    priors = np.array(PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.]), np.float32)
    gen = torch.Generator().manual_seed(3)
    images = torch.rand(2, 299, 299, 3, generator=gen) * 2 - 1
    rng = np.random.RandomState(1)
    n_gt = np.array([3, 0], np.int32)
    gt = np.zeros((2, 13, 4), np.float32)
    xy = rng.uniform(0, .7, (3, 2)); wh = rng.uniform(.05, .3, (3, 2))
    gt[0, :3, :2] = xy; gt[0, :3, 2:] = xy + wh
    res = []
    for use_graph in (True, False):
        net = Net(batch=2, input_size=299, k=5, mode="train", seed=5)
        tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, focal_gamma=2.0, focal_alpha=0.25)
        assert tr.loss.focal == (2.0, 0.25, 0.75)
        tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0
        match = tr.loss.match.cpu().numpy()
        assert (match >= 0).sum(1).tolist() == [3, 0]
        loss2 = tr.loss.loss2.cpu().numpy()
        # the gradient the backward pass started from (grad_scale = 1), against the oracle on the step's own logits and match
        dz = net.d_logits.reshape(2, -1).cpu().numpy()
        logits = net.logits.reshape(2, -1).cpu().numpy()
        ref = FO.focal_loss(tr.loss.decoded.cpu().numpy(), logits, 1, gt, match, 1000.0, 2.0, 0.25, 0.75, 0, 0)
        check_values(dict(loss2=loss2, dl=net.d_locs.reshape(2, -1, 4).cpu().numpy(), dz=dz, n_neg=ref["n_neg"]), ref,
                     "Trainer graph=%d:" % use_graph)
        res.append(loss2)
    assert res[0].tobytes() == res[1].tobytes() and np.isfinite(res[0]).all()
