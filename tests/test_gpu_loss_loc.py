"""GPU: mbx_loss_fwd_bwd_loc (the choice of location term: l2, smooth_l1, giou, diou, ciou, with or without the focal loss and
hard-negative mining) against tests/loc_oracle.py, a float64 restatement whose gradients come from autograd.

The C ABI is driven directly with a hand-made `match` on tests.loc_oracle.make_loc_case (valid gt boxes, positives near
their box: overlapping, inverted and disjoint pairs, none within 1e-5 of a kink -- tests/test_loc_cpu.py counts them).
Bars: the kernel works in float64 and rounds alpha * grad_scale * dL/dl to float32 once, so one float32 rounding (6e-8) and
float64 operation-order noise (under 1e-11 at box sides >= 0.05) is all that separates it from the oracle: gradients
rtol 1e-6 with atol 1e-6 * max|ref|, the location loss rtol 1e-6 (over 10x headroom).  The confidence side (d_logits,
loss2[1], n_neg) is byte-identical to mbx_loss_fwd_bwd_focal on the same arguments, and MBX_LOC_L2 is so in every output.
"""
import numpy as np
import pytest

from tests import loc_oracle as LO
from tests import mined_oracle as MO
from tests.loss_cases import ALPHA, SENTINEL, SHAPES, _forward_backward, batch, call, gpu, make_case, weights  # noqa: F401

pytestmark = pytest.mark.gpu

TYPE = {name: t for t, name in enumerate(LO.TYPES)}          # MBX_LOC_*
GRAD_SCALE = 0.25

# (what, prediction, gt): positives at the kinks of the IoU family, float32-exact or rounded to float32 before use
BOX = [0.2, 0.3, 0.6, 0.7]
DEGENERATE = [("equal", BOX, BOX),
              ("point inside", [0.4, 0.5, 0.4, 0.5], BOX),
              ("point outside", [0.9, 0.9, 0.9, 0.9], BOX),
              ("zero width", [0.3, 0.35, 0.3, 0.65], BOX),
              ("inverted, equal after sorting", [0.6, 0.7, 0.2, 0.3], BOX),
              ("gt of zero area", BOX, [0.4, 0.4, 0.4, 0.4]),
              ("point on a gt of zero area", [0.4, 0.4, 0.4, 0.4], [0.4, 0.4, 0.4, 0.4])]


def call_loc(gpu, c, conf_in, is_logit, loc_type, beta=LO.BETA, gamma=0.0, w=(1.0, 1.0), neg_per_pos=0, min_neg=0, rows=None,
             grad_scale=1.0, ws_short=0, prefill=None):
    """One call of mbx_loss_fwd_bwd_loc on images `rows` of case c -> (status, dict of numpy outputs), as
    tests.loss_cases.call does for the other entries.  loc_type: a name of LO.TYPES or a raw integer."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).cuda()
    dec, x, gt, match = dev(c["dec"]), dev(conf_in), dev(c["gt"]), dev(c["match"])
    B, P, G = match.shape[0], c["P"], c["G"]
    fill = (lambda *s, dt=torch.float32: torch.full(s, prefill, dtype=dt, device="cuda")) if prefill is not None else \
        (lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device="cuda"))
    loss2, dl, dz, n_neg = fill(2), fill(B, P, 4), fill(B, P), fill(B, dt=torch.int32)
    ws = torch.empty((l.mbx_loss_loc_workspace_bytes(B, P),), dtype=torch.uint8, device="cuda")
    st = l.mbx_loss_fwd_bwd_loc(dec.data_ptr(), x.data_ptr(), int(is_logit), gt.data_ptr(), match.data_ptr(), ALPHA, grad_scale,
                                B, P, G, loss2.data_ptr(), dl.data_ptr(), dz.data_ptr(), TYPE.get(loc_type, loc_type), beta,
                                gamma, w[0], w[1], neg_per_pos, min_neg, n_neg.data_ptr(), ws.data_ptr(),
                                ws.numel() - ws_short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, dict(loss2=loss2.cpu().numpy(), dl=dl.cpu().numpy(), dz=dz.cpu().numpy(), n_neg=n_neg.cpu().numpy())


def check_location(out, ref, grad_scale, what=""):
    """The bars of the module docstring on loss2[0] and d_raw_locs; every figure is printed before it is asserted."""
    want = (grad_scale * ref["dl"]).astype(np.float32)        # ref["dl"] = alpha * dL/dl in float64
    top = float(np.abs(want).max()) if want.size else 0.0
    err = np.abs(out["dl"].astype(np.float64) - want) / (1e-6 * top + 1e-6 * np.abs(want) + 1e-300)
    rel = abs(float(out["loss2"][0]) - ref["loc_loss"]) / max(abs(ref["loc_loss"]), 1e-300)
    print("%s loc_loss %r oracle %r rel %.3g; max|dl| %.4g, worst gradient error %.3g x bar" % (
        what, out["loss2"][0], ref["loc_loss"], rel, top, err.max() if err.size else 0.0))
    assert np.isfinite(out["loss2"]).all() and np.isfinite(out["dl"]).all() and np.isfinite(out["dz"]).all()
    assert np.isclose(out["loss2"][0], ref["loc_loss"], rtol=1e-6, atol=0)
    assert np.allclose(out["dl"], want, rtol=1e-6, atol=1e-6 * top)


def same_bytes(a, b, keys=("loss2", "dl", "dz", "n_neg")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def cases():
    out = {s: LO.make_loc_case(*s) for s in SHAPES}
    for s, c in out.items():
        l, g = LO.positives(c)
        # no positive within 1e-5 of a kink: no element is left out of the gradient comparison below
        assert int((LO.kink_distances(l, g, LO.BETA) < 1e-5).sum()) == 0, s
        inverted, disjoint, overlapping = LO.census(l, g)
        assert len(l) < 20 or (inverted >= 1 and disjoint >= 1 and overlapping >= 1), s
    return out


@pytest.fixture(scope="module")
def focal_results(gpu, cases):
    """mbx_loss_fwd_bwd_focal at gamma = 0, weights (1, 1), grad_scale 0.25 on every shape and both input kinds, once."""
    out = {}
    for s, c in cases.items():
        for is_logit in (1, 0):
            st, out[s + (is_logit,)] = call(gpu, c, c["z"] if is_logit else c["x"], is_logit, gamma=0.0, alpha=None,
                                            grad_scale=GRAD_SCALE)
            assert st == 0
    return out


# ------------------------------------------------------------------------------------------ 1. values against the oracle
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
@pytest.mark.parametrize("loc_type", LO.TYPES)
def test_values_against_the_oracle_and_confidence_untouched(gpu, cases, focal_results, B, P, G, is_logit, loc_type):
    c = cases[(B, P, G)]
    x = c["z"] if is_logit else c["x"]
    ref = LO.loc_loss(loc_type, c["dec"], x, is_logit, c["gt"], c["match"], ALPHA)
    st, out = call_loc(gpu, c, x, is_logit, loc_type, grad_scale=GRAD_SCALE)
    assert st == 0
    check_location(out, ref, GRAD_SCALE, "P=%d logit=%d %s:" % (P, is_logit, loc_type))
    assert not out["dl"][c["match"] < 0].any()                # (0, 0, 0, 0) for every prior that is no positive
    if loc_type != "l2":
        assert out["dl"][c["match"] >= 0].any(1).all()        # and something for every positive
    # the confidence side is mbx_loss_fwd_bwd_focal's, byte for byte
    focal = focal_results[(B, P, G, is_logit)]
    assert out["dz"].tobytes() == focal["dz"].tobytes() and out["loss2"][1:].tobytes() == focal["loss2"][1:].tobytes()
    assert np.array_equal(out["n_neg"], focal["n_neg"])


# ------------------------------------------------------------------------------------------------- 2. L2: the old bytes
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
@pytest.mark.parametrize("gamma,alpha", [(0.0, None), (2.0, 0.25)])
@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_l2_is_the_focal_entry_byte_for_byte(gpu, cases, B, P, G, is_logit, gamma, alpha, neg_per_pos):
    c = cases[(B, P, G)]
    x = c["z"] if is_logit else c["x"]
    st_f, focal = call(gpu, c, x, is_logit, gamma=gamma, alpha=alpha, neg_per_pos=neg_per_pos, grad_scale=GRAD_SCALE)
    st_l, loc = call_loc(gpu, c, x, is_logit, "l2", beta=0.0, gamma=gamma, w=weights(alpha), neg_per_pos=neg_per_pos,
                         grad_scale=GRAD_SCALE)               # beta is not looked at for l2
    assert st_f == 0 and st_l == 0
    same_bytes(loc, focal)


# ------------------------------------------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("gamma,alpha,neg_per_pos", [(0.0, None, 3), (2.0, 0.25, 0), (2.0, 0.25, 3)])
def test_giou_composes_with_mining_and_the_focal_loss(gpu, cases, B, P, G, gamma, alpha, neg_per_pos):
    c = cases[(B, P, G)]
    w = weights(alpha)
    st_g, alone = call_loc(gpu, c, c["z"], 1, "giou", grad_scale=GRAD_SCALE)
    st, out = call_loc(gpu, c, c["z"], 1, "giou", gamma=gamma, w=w, neg_per_pos=neg_per_pos, grad_scale=GRAD_SCALE)
    st_f, focal = call(gpu, c, c["z"], 1, gamma=gamma, alpha=alpha, neg_per_pos=neg_per_pos, grad_scale=GRAD_SCALE)
    assert st_g == 0 and st == 0 and st_f == 0
    ref = LO.loc_loss("giou", c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA, gamma=gamma, w_pos=w[0], w_neg=w[1],
                      neg_per_pos=neg_per_pos)
    check_location(out, ref, GRAD_SCALE, "P=%d giou gamma=%g alpha=%r neg_per_pos=%d:" % (P, gamma, alpha, neg_per_pos))
    # the location side does not see the confidence side, and the other way round
    assert out["dl"].tobytes() == alone["dl"].tobytes() and out["loss2"][:1].tobytes() == alone["loss2"][:1].tobytes()
    same_bytes(out, focal, ("dz", "n_neg"))
    assert out["loss2"][1:].tobytes() == focal["loss2"][1:].tobytes()
    # the selection is the mined oracle's
    assert np.array_equal(out["n_neg"], ref["n_neg"])
    neg = c["match"] < 0
    if neg_per_pos:
        mask, K = MO.select(c["z"], c["match"], neg_per_pos, 0)
        assert np.array_equal(ref["mask"], mask) and np.array_equal(out["n_neg"], K)
        assert np.array_equal((out["dz"] != 0) & neg, mask) and np.all(out["dz"].view(np.uint32)[neg & ~mask] == 0)
    else:
        assert np.array_equal(out["n_neg"], P - c["n_pos"]) and np.all(out["dz"][neg] != 0)


# ------------------------------------------------------------------------------------------------ 4. degenerate positives
def _degenerate_case(together):
    """The DEGENERATE pairs as positives: all in image 0 (`together`), or one per image.  P = 200, G = len(DEGENERATE)."""
    n, P = len(DEGENERATE), 200
    B = 1 if together else n
    c = make_case(max(B, 2), P, n)
    c = {k: (v[:B].copy() if isinstance(v, np.ndarray) and k != "n_pos" else v) for k, v in c.items()}
    c["B"] = B
    c["match"][:] = -1
    c["gt"][:] = np.float32(0.5)
    for i, (_, l, g) in enumerate(DEGENERATE):
        b = 0 if together else i
        c["match"][b, 5 + 30 * i] = i                         # priors 5 .. 185: three wavefronts hold them
        c["dec"][b, 5 + 30 * i] = np.array(l, np.float32)
        c["gt"][b, i] = np.array(g, np.float32)
    return c


@pytest.mark.parametrize("loc_type", LO.TYPES)
def test_degenerate_positives_stay_finite_and_follow_the_oracle(gpu, loc_type):
    c = _degenerate_case(together=True)
    ref = LO.loc_loss(loc_type, c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA)
    assert np.isfinite(ref["dl"]).all() and np.isfinite(ref["L"]).all() and len(ref["L"]) == len(DEGENERATE)
    st, out = call_loc(gpu, c, c["z"], 1, loc_type)
    assert st == 0
    for k in ("loss2", "dl", "dz"):
        assert np.isfinite(out[k]).all(), k
    print("%s: loc_loss %r oracle %r" % (loc_type, out["loss2"][0], ref["loc_loss"]))
    assert np.isclose(out["loss2"][0], ref["loc_loss"], rtol=1e-6, atol=0)
    # gradients where the oracle's point is smooth: no kink of the definition within 1e-5
    l, g = LO.positives(c)
    smooth = {"l2": np.ones(len(l), bool), "smooth_l1": (np.abs(np.abs(l - g) - LO.BETA) >= 1e-5).all(1)}.get(
        loc_type, LO.kink_distances(l, g) >= 1e-5)
    b, p = np.nonzero(c["match"] >= 0)
    want = ref["dl"].astype(np.float32)
    top = float(np.abs(want).max())
    print("%s: %d of %d degenerate positives are smooth points" % (loc_type, int(smooth.sum()), len(smooth)))
    assert np.allclose(out["dl"][b[smooth], p[smooth]], want[b[smooth], p[smooth]], rtol=1e-6, atol=1e-6 * top)
    # and at the kinks the conventions of the header (a min or max follows its first argument, max(0, .) passes only
    # where > 0, atan2's derivative is 0 at the origin) are the oracle's too: the whole gradient agrees
    assert np.allclose(out["dl"], want, rtol=1e-6, atol=1e-6 * top)
    # L of each pair alone, through loss2[0] of one-positive images
    each = _degenerate_case(together=False)
    for i, (what, _, _) in enumerate(DEGENERATE):
        st, one = call_loc(gpu, each, each["z"], 1, loc_type, rows=slice(i, i + 1))
        assert st == 0 and np.isfinite(one["loss2"]).all() and np.isfinite(one["dl"]).all()
        print("  %-32s L %r oracle %r" % (what, one["loss2"][0] / ALPHA, ref["L"][i]))
        assert np.isclose(one["loss2"][0], ALPHA * ref["L"][i], rtol=1e-6, atol=0), what


# ------------------------------------------------------------------------------------------------------ 5. rejections
@pytest.mark.parametrize("kw,status", [
    (dict(loc_type=-1), -1), (dict(loc_type=5), -1), (dict(loc_type="smooth_l1", beta=0.0), -1),
    (dict(loc_type="smooth_l1", beta=-0.1), -1), (dict(loc_type="smooth_l1", beta=float("nan")), -1),
    (dict(loc_type="smooth_l1", beta=float("inf")), -1),
    (dict(gamma=-0.5), -1), (dict(gamma=10.5), -1), (dict(gamma=float("nan")), -1), (dict(gamma=float("inf")), -1),
    (dict(w=(-0.25, 1.0)), -1), (dict(w=(1.0, -0.25)), -1), (dict(w=(float("inf"), 1.0)), -1),
    (dict(w=(1.0, float("inf"))), -1), (dict(w=(float("nan"), 1.0)), -1), (dict(w=(1.0, float("nan"))), -1),
    (dict(neg_per_pos=-1), -1), (dict(neg_per_pos=3, min_neg=-1), -1), (dict(neg_per_pos=0, min_neg=1), -1),
    (dict(ws_short=1), -4), (dict(neg_per_pos=3, ws_short=1), -4), (dict(loc_type=5, ws_short=1), -1),
    (dict(loc_type="smooth_l1", beta=0.0, ws_short=1), -1)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, cases, kw, status):
    c = cases[(4, 70, 5)]
    kw = dict(dict(loc_type="giou"), **kw)
    st, out = call_loc(gpu, c, c["z"], 1, prefill=SENTINEL, **kw)
    assert st == status
    assert np.all(out["loss2"] == SENTINEL) and np.all(out["dl"] == SENTINEL) and np.all(out["dz"] == SENTINEL)
    assert np.all(out["n_neg"] == int(SENTINEL))


def test_a_good_call_writes_every_buffer_and_beta_is_ignored_off_smooth_l1(gpu, cases):
    c = cases[(4, 70, 5)]
    st, out = call_loc(gpu, c, c["z"], 1, "giou", prefill=SENTINEL)
    assert st == 0 and not np.any(out["dz"] == SENTINEL) and not np.any(out["n_neg"] == int(SENTINEL))
    assert not np.any(out["loss2"] == SENTINEL) and not np.any(out["dl"] == SENTINEL)
    for beta in (0.0, -1.0, float("nan")):
        for t in ("l2", "giou", "diou", "ciou"):
            st_a, a = call_loc(gpu, c, c["z"], 1, t, beta=beta)
            st_b, b = call_loc(gpu, c, c["z"], 1, t)
            assert st_a == 0 and st_b == 0
            same_bytes(a, b)


def test_what_the_plain_entry_rejects_is_rejected_and_null_outputs_are_taken(gpu, cases):
    torch, l = gpu
    c = cases[(4, 70, 5)]
    t = {k: torch.from_numpy(c[k]).cuda() for k in ("dec", "z", "gt", "match")}
    loss2 = torch.full((2,), SENTINEL, device="cuda")
    ws = torch.empty((l.mbx_loss_loc_workspace_bytes(4, 70),), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def go(dec=t["dec"].data_ptr(), z=t["z"].data_ptr(), gt=t["gt"].data_ptr(), match=t["match"].data_ptr(),
           out=loss2.data_ptr(), B=4, P=70, G=5, w=ws.data_ptr(), neg_per_pos=0):
        return l.mbx_loss_fwd_bwd_loc(dec, z, 1, gt, match, ALPHA, 1.0, B, P, G, out, None, None, TYPE["ciou"], 0.0, 2.0, 0.25,
                                      0.75, neg_per_pos, 0, None, w, ws.numel(), s)
    for kw in (dict(dec=None), dict(z=None), dict(gt=None), dict(match=None), dict(out=None), dict(B=0), dict(B=-1),
               dict(P=0), dict(G=0)):
        assert go(**kw) == -1, kw
    assert go(w=None) == -4
    torch.cuda.synchronize()
    assert np.all(loss2.cpu().numpy() == SENTINEL)
    w_pos, w_neg = 0.25, 0.75
    for neg_per_pos in (0, 3):                                # d_raw_locs, d_logits and n_neg may all be NULL
        assert go(neg_per_pos=neg_per_pos) == 0
        torch.cuda.synchronize()
        ref = LO.loc_loss("ciou", c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA, gamma=2.0, w_pos=w_pos, w_neg=w_neg,
                          neg_per_pos=neg_per_pos)
        got = loss2.cpu().numpy()
        assert np.isclose(got[0], ref["loc_loss"], rtol=1e-6, atol=0) and np.isclose(got[1], ref["conf_loss"], rtol=1e-5)


# ------------------------------------------------------------------------------------------- 6. through MultiboxLoss
def test_multibox_loss_without_the_switch_is_unchanged_and_l2_is_its_bytes(gpu, batch):
    torch, _ = gpu
    from multibox_amd import loss as L
    for kw in (dict(), dict(neg_per_pos=3, min_neg=2), dict(focal_gamma=2.0, focal_alpha=0.25),
               dict(match_iou_threshold=0.3, focal_gamma=0.5, neg_per_pos=3)):
        old = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, **kw)            # the call as it always was
        new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, loc_loss=None, loc_beta=None, **kw)
        l2 = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, loc_loss="l2", **kw)
        assert new.loc is None and new.entry == old.entry and new.entry_args[:-1] == old.entry_args[:-1]
        assert new.ws.numel() == old.ws.numel() and l2.entry == "mbx_loss_fwd_bwd_loc"
        a, b, c = (_forward_backward(torch, m, batch) for m in (old, new, l2))
        for x, y, z in zip(a, b, c):
            assert x.tobytes() == y.tobytes() and x.tobytes() == z.tobytes()
        if old.n_neg is not None:
            assert torch.equal(old.n_neg, new.n_neg) and torch.equal(old.n_neg, l2.n_neg)


@pytest.mark.parametrize("kw", [dict(loc_loss="giou"), dict(loc_loss="smooth_l1", match_iou_threshold=0.3),
                                dict(loc_loss="ciou", focal_gamma=2.0, focal_alpha=0.25, neg_per_pos=3, min_neg=2)])
def test_multibox_loss_with_the_real_matcher(gpu, batch, kw):
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
    w_pos, w_neg = weights(kw.get("focal_alpha"))
    ref = LO.loc_loss(kw["loc_loss"], ml.decoded.cpu().numpy(), batch["logits"], 1, batch["gt"], match, ALPHA,
                      gamma=kw.get("focal_gamma", 0.0), w_pos=w_pos, w_neg=w_neg, neg_per_pos=kw.get("neg_per_pos", 0),
                      min_neg=kw.get("min_neg", 0))
    check_location(dict(loss2=loss2, dl=dl, dz=dz), ref, 1.0, "MultiboxLoss %r:" % (kw,))
    assert not dl[match < 0].any()
    # the match (its cost stays the reference's) and the confidence side are those of the object without the location switch
    rest = {k: v for k, v in kw.items() if k != "loc_loss"}
    other = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, **rest)
    o_loss2, _, o_dz = _forward_backward(torch, other, batch)
    assert np.array_equal(other.match.cpu().numpy(), match)
    assert o_dz.tobytes() == dz.tobytes() and o_loss2[1:].tobytes() == loss2[1:].tobytes()
    if "neg_per_pos" in kw:
        assert np.array_equal(ml.n_neg.cpu().numpy(), ref["n_neg"])
    else:
        assert ml.n_neg is None


# --------------------------------------------------------------------------------------------- 7. through the Trainer
def test_trainer_step_ciou_graph_equals_eager(gpu):
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
        tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, loc_loss="ciou")
        assert tr.loss.loc == (TYPE["ciou"], 0.0) and tr.loss.entry == "mbx_loss_fwd_bwd_loc"
        tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0
        match = tr.loss.match.cpu().numpy()
        assert (match >= 0).sum(1).tolist() == [3, 0]
        loss2 = tr.loss.loss2.cpu().numpy()
        # the gradient the backward pass started from (grad_scale = 1), against the oracle on the step's own boxes and match
        logits = net.logits.reshape(2, -1).cpu().numpy()
        ref = LO.loc_loss("ciou", tr.loss.decoded.cpu().numpy(), logits, 1, gt, match, 1000.0)
        check_location(dict(loss2=loss2, dl=net.d_locs.reshape(2, -1, 4).cpu().numpy(), dz=net.d_logits.reshape(2, -1).cpu().numpy()),
                       ref, 1.0, "Trainer graph=%d:" % use_graph)
        assert np.isclose(loss2[1], ref["conf_loss"], rtol=1e-5)
        res.append(loss2)
    assert res[0].tobytes() == res[1].tobytes() and np.isfinite(res[0]).all()
