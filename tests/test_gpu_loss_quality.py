"""GPU: mbx_loss_fwd_bwd_quality (the IoU as the positives' confidence target: quality focal loss and varifocal loss, with any
location term, with or without hard-negative mining) against tests/quality_oracle.py.

The C ABI is driven directly with the hand-made `match` of tests.loc_oracle.make_loc_case, like test_gpu_loss_loc.py.  Bars:
the confidence side's own from test_gpu_loss_focal.py -- the selection and n_neg exact, losses rtol 1e-5, gradients rtol 1e-4 /
atol 1e-6 (times |grad_scale| where that is under 1): s, c, w are float32 and the device's expf is not numpy's, which tests/test_quality_cpu.py
shows to move a gradient by at most 0.12 of that bar on these inputs; q_stats: the count exact, the sum rtol 1e-12 (float64
sums of the same numbers in another order).  MBX_QUALITY_NONE, the location side, n_neg and the negatives' d_logits are held to
mbx_loss_fwd_bwd_loc byte for byte."""
import numpy as np
import pytest

from tests import atss_cases as AC
from tests import loc_oracle as LO
from tests import mined_oracle as MO
from tests import quality_oracle as QO
from tests.loss_cases import ALPHA, SENTINEL, SHAPES, _forward_backward, batch, gpu, make_case  # noqa: F401
from tests.test_gpu_loss_loc import TYPE, call_loc, same_bytes

pytestmark = pytest.mark.gpu

GRAD_SCALE = 0.25


def call_q(gpu, c, conf_in, is_logit, quality, loc_type="l2", beta=LO.BETA, gamma=2.0, w=(1.0, 1.0), neg_per_pos=0, min_neg=0,
           rows=None, grad_scale=1.0, ws_short=0, prefill=None, stats=True):
    """One call of mbx_loss_fwd_bwd_quality on images `rows` of case c -> (status, dict of numpy outputs), as
    tests.test_gpu_loss_loc.call_loc does for its entry.  quality: a name of QO.QUALITY or a raw integer."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).cuda()
    dec, x, gt, match = dev(c["dec"]), dev(conf_in), dev(c["gt"]), dev(c["match"])
    B, P, G = match.shape[0], c["P"], c["G"]
    fill = (lambda *s, dt=torch.float32: torch.full(s, prefill, dtype=dt, device="cuda")) if prefill is not None else \
        (lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device="cuda"))
    loss2, dl, dz, n_neg, qs = fill(2), fill(B, P, 4), fill(B, P), fill(B, dt=torch.int32), fill(B, 2, dt=torch.float64)
    ws = torch.empty((l.mbx_loss_quality_workspace_bytes(B, P),), dtype=torch.uint8, device="cuda")
    st = l.mbx_loss_fwd_bwd_quality(dec.data_ptr(), x.data_ptr(), int(is_logit), gt.data_ptr(), match.data_ptr(), ALPHA,
                                    grad_scale, B, P, G, loss2.data_ptr(), dl.data_ptr(), dz.data_ptr(),
                                    TYPE.get(loc_type, loc_type), beta, QO.QUALITY.get(quality, quality), gamma, w[0], w[1],
                                    neg_per_pos, min_neg, n_neg.data_ptr(), qs.data_ptr() if stats else None, ws.data_ptr(),
                                    ws.numel() - ws_short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, dict(loss2=loss2.cpu().numpy(), dl=dl.cpu().numpy(), dz=dz.cpu().numpy(), n_neg=n_neg.cpu().numpy(),
                    q_stats=qs.cpu().numpy())


def check_confidence(out, ref, grad_scale, what=""):
    """The bars of the module docstring on loss2[1], d_logits, n_neg and q_stats; every figure is printed before it is
    asserted."""
    want = grad_scale * ref["d_conf_in"]
    atol = 1e-6 * min(1.0, abs(grad_scale))                   # never wider than the bar at grad_scale = 1
    err = np.abs(out["dz"].astype(np.float64) - want) / (atol + 1e-4 * np.abs(want))
    rel = abs(float(out["loss2"][1]) - ref["conf_loss"]) / max(abs(ref["conf_loss"]), 1e-300)
    q_rel = np.abs(out["q_stats"][:, 0] - ref["q_stats"][:, 0]) / np.maximum(np.abs(ref["q_stats"][:, 0]), 1e-300)
    print("%s conf_loss %r oracle %r rel %.3g; worst gradient error %.3g x bar; q sums %s oracle %s worst rel %.3g; counts %s" % (
        what, out["loss2"][1], ref["conf_loss"], rel, err.max(), out["q_stats"][:, 0].tolist(), ref["q_stats"][:, 0].tolist(),
        q_rel.max(), out["q_stats"][:, 1].tolist()))
    assert np.isfinite(out["loss2"]).all() and np.isfinite(out["dz"]).all() and np.isfinite(out["q_stats"]).all()
    assert np.array_equal(out["n_neg"], ref["n_neg"])
    assert np.isclose(out["loss2"][1], ref["conf_loss"], rtol=1e-5, atol=0)
    assert np.allclose(out["dz"], want, rtol=1e-4, atol=atol)
    assert np.array_equal(out["q_stats"][:, 1], ref["q_stats"][:, 1])
    assert np.allclose(out["q_stats"][:, 0], ref["q_stats"][:, 0], rtol=1e-12, atol=0)


def check_location(out, ref, grad_scale):
    """loss2[0] and d_raw_locs at test_gpu_loss_loc.py's bars (l2 runs the float32 lines: ref_numpy's own rounding)."""
    want = (grad_scale * ref["dl"]).astype(np.float32)
    top = float(np.abs(want).max()) if want.size else 0.0
    assert np.isclose(out["loss2"][0], ref["loc_loss"], rtol=1e-6, atol=0)
    assert np.allclose(out["dl"], want, rtol=1e-6, atol=1e-6 * top)


@pytest.fixture(scope="module")
def cases():
    return {s: LO.make_loc_case(*s) for s in SHAPES}


# ------------------------------------------------------------------------------------------ 1. values against the oracle
VALUE_CASES = [(mode, gamma, is_logit, neg_per_pos, loc_type)
               for mode in QO.MODES for gamma in ((0.0, 1.0, 2.0, 5.0) if mode == "qfl" else (0.0, 2.0, 5.0))
               for is_logit in (1, 0) for neg_per_pos in (0, 3) for loc_type in ("l2", "giou")]


@pytest.mark.parametrize("B,P,G", SHAPES)
def test_values_against_the_oracle(gpu, cases, B, P, G):
    c = cases[(B, P, G)]
    for i, (mode, gamma, is_logit, neg_per_pos, loc_type) in enumerate(VALUE_CASES):
        x = c["z"] if is_logit else c["x"]
        w = (1.0, 1.0) if mode == "qfl" else (1.0, 0.75)
        grad_scale = (1.0, GRAD_SCALE, -2.0)[i % 3]
        ref = QO.quality_loss(mode, loc_type, c["dec"], x, is_logit, c["gt"], c["match"], ALPHA, gamma, w[0], w[1], neg_per_pos)
        # the census: a changed fixture fails here, loudly
        assert (ref["q"] == 0).any() and ((ref["q"] > 0.3) & (ref["q"] < 0.95)).any() and np.abs(ref["q"] - ref["s"]).min() >= 1e-3
        st, out = call_q(gpu, c, x, is_logit, mode, loc_type, gamma=gamma, w=w, neg_per_pos=neg_per_pos, grad_scale=grad_scale)
        assert st == 0
        check_confidence(out, ref, grad_scale, "P=%d %s gamma=%g logit=%d neg_per_pos=%d %s scale=%g:" % (
            P, mode, gamma, is_logit, neg_per_pos, loc_type, grad_scale))
        check_location(out, ref, grad_scale)
        neg = c["match"] < 0
        if neg_per_pos:                                       # the selection is the mined oracle's, exactly
            mask, K = MO.select(x, c["match"], neg_per_pos, 0)
            assert np.array_equal(ref["mask"], mask) and np.array_equal(out["n_neg"], K)
            assert np.array_equal((out["dz"] != 0) & neg, mask) and np.all(out["dz"].view(np.uint32)[neg & ~mask] == 0)
        else:
            assert np.array_equal(out["n_neg"], P - c["n_pos"])


# ------------------------------------------------------------------ 2. MBX_QUALITY_NONE: mbx_loss_fwd_bwd_loc's bytes
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("loc_type", ["l2", "giou"])
@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_quality_none_is_the_loc_entry_byte_for_byte(gpu, cases, B, P, G, loc_type, gamma, neg_per_pos):
    c = cases[(B, P, G)]
    kw = dict(gamma=gamma, w=(0.25, 0.75), neg_per_pos=neg_per_pos, grad_scale=GRAD_SCALE)
    st_l, loc = call_loc(gpu, c, c["z"], 1, loc_type, **kw)
    st_q, out = call_q(gpu, c, c["z"], 1, "none", loc_type, stats=False, **kw)
    assert st_l == 0 and st_q == 0
    same_bytes(out, loc)


# ------------------------------------------------------------------------------- 3. what the mode must not touch
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("mode", QO.MODES)
@pytest.mark.parametrize("loc_type,neg_per_pos,grad_scale", [("l2", 0, GRAD_SCALE), ("giou", 3, -GRAD_SCALE), ("ciou", 3, 1.0)])
def test_the_location_side_n_neg_and_the_negatives_are_the_loc_entrys_bytes(gpu, cases, B, P, G, mode, loc_type, neg_per_pos,
                                                                            grad_scale):
    c = cases[(B, P, G)]
    kw = dict(gamma=2.0, w=(1.0, 0.75), neg_per_pos=neg_per_pos, grad_scale=grad_scale)
    st_l, loc = call_loc(gpu, c, c["z"], 1, loc_type, **kw)
    st_q, out = call_q(gpu, c, c["z"], 1, mode, loc_type, **kw)
    assert st_l == 0 and st_q == 0
    assert out["loss2"][:1].tobytes() == loc["loss2"][:1].tobytes()
    same_bytes(out, loc, ("dl", "n_neg"))
    neg = c["match"] < 0
    assert out["dz"][neg].tobytes() == loc["dz"][neg].tobytes()
    if neg_per_pos:
        mask, _ = MO.select(c["z"], c["match"], neg_per_pos, 0)
        assert (neg & ~mask).any() and np.all(out["dz"].view(np.uint32)[neg & ~mask] == 0)     # +0 whatever grad_scale's sign
    pos_differs = out["dz"][~neg] != loc["dz"][~neg]
    assert pos_differs.size == 0 or pos_differs.any()         # and the positives are another loss


# ---------------------------------------------------------------------------------------------- 4. edges, hand-made
BOX = [0.2, 0.3, 0.6, 0.7]
# (what, prediction, gt, logit)
EDGES = [("equal", BOX, BOX, 0.5), ("equal, high score", BOX, BOX, 8.0), ("disjoint", [0.7, 0.8, 0.9, 0.95], BOX, 1.0),
         ("touching", [0.6, 0.3, 0.8, 0.7], BOX, -1.0), ("inverted", [0.55, 0.3, 0.25, 0.7], BOX, 0.25),
         ("zero width", [0.3, 0.35, 0.3, 0.65], BOX, -0.5), ("point", [0.4, 0.5, 0.4, 0.5], BOX, 2.0),
         ("overlapping", [0.3, 0.35, 0.7, 0.8], BOX, -8.0),
         ("equal, logit 200", BOX, BOX, 200.0), ("equal, logit -200", BOX, BOX, -200.0), ("overlapping, logit 30", [0.3, 0.35, 0.7, 0.8], BOX, 30.0),
         ("overlapping, logit -30", [0.3, 0.35, 0.7, 0.8], BOX, -30.0), ("disjoint, logit 200", [0.7, 0.8, 0.9, 0.95], BOX, 200.0),
         ("disjoint, logit -200: q == s", [0.7, 0.8, 0.9, 0.95], BOX, -200.0)]


def _edge_case():
    """The EDGES as the positives of one image: P = 450, priors 5, 35, ...: several wavefronts hold them."""
    n, P = len(EDGES), 450
    c = make_case(2, P, n)
    c = {k: (v[:1].copy() if isinstance(v, np.ndarray) and k != "n_pos" else v) for k, v in c.items()}
    c["B"] = 1
    c["match"][:] = -1
    c["gt"][:] = np.float32(0.5)
    at = 5 + 30 * np.arange(n)
    for i, (_, l, g, z) in enumerate(EDGES):
        c["match"][0, at[i]] = i
        c["dec"][0, at[i]], c["gt"][0, i], c["z"][0, at[i]] = np.array(l, np.float32), np.array(g, np.float32), np.float32(z)
    return c, at


@pytest.mark.parametrize("mode,gamma", [("qfl", 0.0), ("qfl", 1.0), ("qfl", 2.0), ("qfl", 5.0), ("varifocal", 2.0)])
def test_edges_stay_finite_and_follow_the_oracle(gpu, mode, gamma):
    c, at = _edge_case()
    w = (1.0, 0.75)
    ref = QO.quality_loss(mode, "giou", c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA, gamma, *w)
    q = dict(zip((e[0] for e in EDGES), ref["q"]))
    assert np.isfinite(ref["d_conf_in"]).all() and np.isfinite(ref["L"]).all()
    assert 1 - 1e-6 < q["equal"] < 1 and q["disjoint"] == 0 and q["touching"] == 0 and q["zero width"] == 0 and q["point"] == 0
    assert 0 < q["inverted"] < 1 and 0 < q["overlapping"] < 1
    st, out = call_q(gpu, c, c["z"], 1, mode, "giou", gamma=gamma, w=w)
    assert st == 0
    for k in ("loss2", "dl", "dz", "q_stats"):
        assert np.isfinite(out[k]).all(), k
    got, want = out["dz"][0, at].astype(np.float64), ref["d_conf_in"][0, at]
    for (what, _, _, z), g_, w_, L_ in zip(EDGES, got, want, ref["L"]):
        print("%-32s %s gamma=%g: d_logits %r oracle %r, oracle term %r" % (what, mode, gamma, g_, w_, L_))
    moderate = np.array([abs(e[3]) <= 8 for e in EDGES])
    assert np.allclose(got[moderate], want[moderate], rtol=1e-4, atol=1e-6)
    # the saturated ones: the float32 s is an ulp-sensitive input there -- finiteness (above) and sign
    sign = lambda a: np.sign(np.where(np.abs(a) < 1e-30, 0.0, a))
    assert np.all((sign(got[~moderate]) == sign(want[~moderate])) | (np.abs(want[~moderate]) < 1e-6))
    assert out["q_stats"][0, 1] == len(EDGES) and np.isclose(out["q_stats"][0, 0], ref["q"].sum(), rtol=1e-12)
    # q == 0 and s == 0 exactly: the term and the gradient are exactly 0 under qfl with gamma >= 1 and under varifocal
    if gamma:
        assert got[-1] == 0 and ref["L"][-1] == 0
        only = dict(c, match=np.where(np.arange(c["P"]) == at[-1], c["match"], -1).astype(np.int32))
        st, one = call_q(gpu, only, c["z"], 1, mode, "giou", gamma=gamma, w=(1.0, 0.0))      # w_neg = 0: the one positive's term alone
        assert st == 0 and one["loss2"][1] == 0 and one["dz"][0, at[-1]] == 0
    if mode == "varifocal":                                   # q == 0: neither loss nor gradient, whatever the score
        zero = np.array([e[0] in ("disjoint", "touching", "zero width", "point", "disjoint, logit 200") for e in EDGES])
        assert np.all(got[zero] == 0) and np.all(ref["L"][zero] == 0)


# ------------------------------------------------------------------------ 5. row independence and repeatability
@pytest.mark.parametrize("mode,neg_per_pos", [("qfl", 0), ("varifocal", 3)])
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, cases, mode, neg_per_pos):
    c = cases[(4, 646, 13)]
    kw = dict(loc_type="giou", gamma=2.0, w=(1.0, 0.75), neg_per_pos=neg_per_pos, grad_scale=GRAD_SCALE)
    st, whole = call_q(gpu, c, c["z"], 1, mode, **kw)
    st2, again = call_q(gpu, c, c["z"], 1, mode, **kw)
    assert st == 0 and st2 == 0
    same_bytes(whole, again, ("loss2", "dl", "dz", "n_neg", "q_stats"))
    for b in range(4):
        st, alone = call_q(gpu, c, c["z"], 1, mode, rows=slice(b, b + 1), **kw)
        assert st == 0
        for k in ("dl", "dz", "n_neg", "q_stats"):
            assert alone[k][0].tobytes() == whole[k][b].tobytes(), (k, b)
    st, moved = call_q(gpu, c, c["z"], 1, mode, rows=[3, 2, 1, 0, 2], **kw)      # another place in a larger launch
    assert st == 0
    for k in ("dl", "dz", "n_neg", "q_stats"):
        for i, b in enumerate([3, 2, 1, 0, 2]):
            assert moved[k][i].tobytes() == whole[k][b].tobytes(), (k, b)


# ------------------------------------------------------------------------------------- 6. refusals write nothing
@pytest.mark.parametrize("kw,status", [
    (dict(quality=-1), -1), (dict(quality=3), -1), (dict(quality="qfl", gamma=0.5), -1), (dict(quality="qfl", gamma=0.999), -1),
    (dict(gamma=-0.5), -1), (dict(gamma=10.5), -1), (dict(gamma=float("nan")), -1), (dict(quality="varifocal", gamma=float("nan")), -1),
    (dict(quality="none"), -1),                               # q_stats with MBX_QUALITY_NONE
    (dict(loc_type=5), -1), (dict(loc_type="smooth_l1", beta=0.0), -1), (dict(w=(-1.0, 1.0)), -1), (dict(w=(1.0, float("inf"))), -1),
    (dict(neg_per_pos=-1), -1), (dict(neg_per_pos=0, min_neg=1), -1),
    (dict(ws_short=1), -4), (dict(quality="varifocal", neg_per_pos=3, ws_short=1), -4), (dict(quality="none", stats=False, ws_short=1), -4),
    (dict(quality=3, ws_short=1), -1), (dict(quality="qfl", gamma=0.5, ws_short=1), -1), (dict(quality="none", ws_short=1), -1)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, cases, kw, status):
    c = cases[(4, 70, 5)]
    kw = dict(dict(quality="qfl", loc_type="giou"), **kw)
    st, out = call_q(gpu, c, c["z"], 1, prefill=SENTINEL, **kw)
    assert st == status
    for k in ("loss2", "dl", "dz", "q_stats"):
        assert np.all(out[k] == SENTINEL), k
    assert np.all(out["n_neg"] == int(SENTINEL))


def test_a_good_call_writes_every_buffer_and_null_outputs_are_taken(gpu, cases):
    torch, l = gpu
    c = cases[(4, 70, 5)]
    for mode in QO.MODES:
        st, out = call_q(gpu, c, c["z"], 1, mode, "giou", prefill=SENTINEL)
        assert st == 0
        for k in ("loss2", "dl", "dz", "q_stats"):
            assert not np.any(out[k] == SENTINEL), k
        assert not np.any(out["n_neg"] == int(SENTINEL))
    t = {k: torch.from_numpy(c[k]).cuda() for k in ("dec", "z", "gt", "match")}
    loss2 = torch.full((2,), SENTINEL, device="cuda")
    ws = torch.empty((l.mbx_loss_quality_workspace_bytes(4, 70),), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def go(dec=t["dec"].data_ptr(), z=t["z"].data_ptr(), gt=t["gt"].data_ptr(), match=t["match"].data_ptr(),
           out=loss2.data_ptr(), B=4, P=70, G=5, w=ws.data_ptr(), neg_per_pos=0, quality=2):
        return l.mbx_loss_fwd_bwd_quality(dec, z, 1, gt, match, ALPHA, 1.0, B, P, G, out, None, None, TYPE["ciou"], 0.0, quality,
                                          2.0, 1.0, 0.75, neg_per_pos, 0, None, None, w, ws.numel(), s)
    for kw in (dict(dec=None), dict(z=None), dict(gt=None), dict(match=None), dict(out=None), dict(B=0), dict(B=-1),
               dict(P=0), dict(G=0)):
        assert go(**kw) == -1, kw
    assert go(w=None) == -4
    torch.cuda.synchronize()
    assert np.all(loss2.cpu().numpy() == SENTINEL)
    for neg_per_pos in (0, 3):                                # d_raw_locs, d_logits, n_neg and q_stats may all be NULL
        for quality in (0, 1, 2):
            assert go(neg_per_pos=neg_per_pos, quality=quality) == 0
            torch.cuda.synchronize()
            got = loss2.cpu().numpy()
            if quality:
                ref = QO.quality_loss(QO.MODES[quality - 1], "ciou", c["dec"], c["z"], 1, c["gt"], c["match"], ALPHA, 2.0, 1.0,
                                      0.75, neg_per_pos)
                assert np.isclose(got[0], ref["loc_loss"], rtol=1e-6, atol=0) and np.isclose(got[1], ref["conf_loss"], rtol=1e-5)


# ------------------------------------------------------------------------------------- 7. through MultiboxLoss
def test_multibox_loss_without_the_switch_is_unchanged(gpu, batch):
    torch, _ = gpu
    from multibox_amd import loss as L
    for kw in (dict(), dict(neg_per_pos=3, min_neg=2), dict(focal_gamma=2.0, focal_alpha=0.25), dict(loc_loss="giou", neg_per_pos=3)):
        old = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, **kw)            # the call as it always was
        new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, quality_target=None, quality_gamma=None,
                             quality_neg_weight=None, **kw)
        assert new.quality is None and new.q_stats is None and new.entry == old.entry and new.ws.numel() == old.ws.numel()
        assert new.entry != "mbx_loss_fwd_bwd_quality" and len(new.entry_args) == len(old.entry_args)
        for x, y in zip(_forward_backward(torch, old, batch), _forward_backward(torch, new, batch)):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("kw", [dict(quality_target="qfl"), dict(quality_target="varifocal"),
                                dict(quality_target="qfl", loc_loss="giou", atss_topk=9, neg_per_pos=3, min_neg=2),
                                dict(quality_target="varifocal", quality_gamma=1.5, quality_neg_weight=0.5, loc_loss="giou",
                                     atss_topk=9, neg_per_pos=3)])
def test_multibox_loss_with_the_real_matcher(gpu, batch, kw):
    torch, _ = gpu
    from multibox_amd import loss as L
    if "atss_topk" in kw:
        kw = dict(kw, prior_levels=AC.LEVELS_299)
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, **kw)
    assert ml.entry == "mbx_loss_fwd_bwd_quality"
    loss2, dl, dz = _forward_backward(torch, ml, batch)
    match = ml.match.cpu().numpy()
    n_matched = (match >= 0).sum(1)
    if "atss_topk" in kw:
        n_atss = ml.n_atss.cpu().numpy()
        assert np.array_equal(n_matched, batch["n"] + n_atss) and n_atss.sum() > 0           # the extended match is what is read
    else:
        assert np.array_equal(n_matched, batch["n"])
    mode = kw["quality_target"]
    ref = QO.quality_loss(mode, kw.get("loc_loss", "l2"), ml.decoded.cpu().numpy(), batch["logits"], 1, batch["gt"], match, ALPHA,
                          kw.get("quality_gamma", 2.0), 1.0, kw.get("quality_neg_weight", L.QUALITY_NEG_WEIGHT_DEFAULT[mode]),
                          kw.get("neg_per_pos", 0), kw.get("min_neg", 0))
    n_neg = ml.n_neg.cpu().numpy() if ml.n_neg is not None else ref["n_neg"]
    check_confidence(dict(loss2=loss2, dz=dz, n_neg=n_neg, q_stats=ml.q_stats.cpu().numpy()), ref, 1.0, "MultiboxLoss %r:" % (kw,))
    check_location(dict(loss2=loss2, dl=dl), ref, 1.0)
    assert ml.q_stats[1].tolist() == [0.0, 0.0]               # the image without boxes


# ------------------------------------------------------------------------------------------ 8. through the Trainer
def test_trainer_step_qfl_graph_equals_eager(gpu):
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
        tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, quality_target="qfl")
        assert tr.loss.quality == (1, 2.0, 1.0, 1.0) and tr.loss.entry == "mbx_loss_fwd_bwd_quality"
        tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0
        match = tr.loss.match.cpu().numpy()
        assert (match >= 0).sum(1).tolist() == [3, 0]
        loss2 = tr.loss.loss2.cpu().numpy()
        d_locs, d_logits = net.d_locs.reshape(2, -1, 4).cpu().numpy(), net.d_logits.reshape(2, -1).cpu().numpy()
        # the gradient the backward pass started from (grad_scale = 1), against the oracle on the step's own boxes and match
        ref = QO.quality_loss("qfl", "l2", tr.loss.decoded.cpu().numpy(), net.logits.reshape(2, -1).cpu().numpy(), 1, gt, match,
                              1000.0, 2.0)
        check_confidence(dict(loss2=loss2, dz=d_logits, n_neg=ref["n_neg"], q_stats=tr.loss.q_stats.cpu().numpy()), ref, 1.0,
                         "Trainer graph=%d:" % use_graph)
        check_location(dict(loss2=loss2, dl=d_locs), ref, 1.0)
        iou = tr.mean_positive_iou()
        print("mean positive IoU %r" % (iou,))
        assert 0.0 <= iou <= 1.0 and np.isclose(iou, ref["q"].mean(), rtol=1e-12, atol=1e-300)
        res.append((loss2, d_locs, d_logits, tr.loss.q_stats.cpu().numpy()))
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


def test_trainer_without_the_key_reports_none_and_picks_the_parents_entry(gpu):
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer
    from multibox_amd import priors as PR
    priors = np.array(PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.]), np.float32)
    tr = Trainer(Net(batch=2, input_size=299, k=5, mode="train", seed=5), priors, max_num_bboxes=13, use_graph=False)
    assert tr.mean_positive_iou() is None and tr.loss.q_stats is None
    assert tr.loss.entry == "mbx_loss_fwd_bwd" and tr.loss.entry_args == ()
