"""GPU: mbx_loss_fwd_bwd_mined (hard-negative mining of the confidence loss) against tests/mined_oracle.py.

The C ABI is driven directly with a hand-made `match`, so nothing here depends on the matcher.  Bars: the selection
(which negatives count, n_neg, the +0 gradients of the others) is exact; loss values rtol 1e-5, gradients rtol 1e-4 /
atol 1e-6 (the bars of mbx_loss_fwd_bwd in test_gpu_postproc.py); K = N_neg is byte-identical to mbx_loss_fwd_bwd.
"""
import numpy as np
import pytest

from tests import mined_oracle as MO
from tests import loss_cases as LC
from tests.loss_cases import ALPHA, SENTINEL, SHAPES, _forward_backward, batch, cut_splits_a_run, gpu, make_case  # noqa: F401

pytestmark = pytest.mark.gpu


def call(gpu, c, conf_in, is_logit, neg_per_pos=3, min_neg=0, mined=True, **kw):
    """loss_cases.call on the mined entry, neg_per_pos = 3 unless said; mined=False: on the plain entry."""
    return LC.call(gpu, c, conf_in, is_logit, entry="mined" if mined else "plain", neg_per_pos=neg_per_pos, min_neg=min_neg,
                   **kw)


def check_selection(c, out, mask, K):
    """With conf_is_logit = 0 a selected negative's gradient is 1/w != 0, so d_logits shows the selection."""
    neg = c["match"] < 0
    assert np.array_equal(out["n_neg"], K)
    assert np.array_equal((out["dz"] != 0) & neg, mask)
    assert np.all(out["dz"].view(np.uint32)[neg & ~mask] == 0)            # +0.0f by bits
    assert np.all(out["dz"][~neg] < 0)                                    # positives: -1/c


# ------------------------------------------------------------------------------------------------- selection is exact
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("kind,min_neg", [("plain", 0), ("plain", 5), ("quantised", 0), ("zeros", None)])
def test_selection_is_exact(gpu, B, P, G, kind, min_neg):
    c = make_case(B, P, G, kind)
    min_neg = P // 2 if min_neg is None else min_neg          # zeros: the cut has to reach the run of zeros
    mask, K = MO.select(c["x"], c["match"], 3, min_neg)
    assert K[0] == min(P, min_neg)                            # the image without positives
    assert K[1] == min(P - min(G, P), max(min_neg, 3 * min(G, P)))
    if (B, P, G) == (3, 13, 13):
        assert K[1] == 0 and not (c["match"][1] < 0).any()    # no negative at all
    st, out = call(gpu, c, c["x"], 0, 3, min_neg)
    assert st == 0
    check_selection(c, out, mask, K)
    if kind == "quantised" and P >= 70:
        # the cut falls inside a run of equal keys: only the index rule decides there
        assert cut_splits_a_run(c, mask)
    if kind == "zeros" and P >= 70:
        hit = cut_splits_a_run(c, mask)
        assert hit
        zero_bits = {int(v) for b in hit for v in c["x"][b][(c["match"][b] < 0) & mask[b] & (c["x"][b] == 0)].view(np.uint32)}
        assert zero_bits == {0, 0x80000000}                   # -0.0 and +0.0 are one run
    if min_neg == 0:
        assert not out["dz"][0].any()                         # no positive, min_neg = 0: the whole row is zero
        st1, alone = call(gpu, c, c["x"], 0, 3, 0, rows=slice(0, 1))
        assert st1 == 0 and alone["n_neg"][0] == 0
        assert alone["loss2"].view(np.uint32).tolist() == [0, 0]      # and it adds exactly nothing to either loss


# ------------------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("is_logit", [1, 0])
def test_values_against_the_oracle(gpu, B, P, G, is_logit):
    c = make_case(B, P, G)
    x = c["z"] if is_logit else c["x"]
    ref = MO.mined_loss(c["dec"], x, is_logit, c["gt"], c["match"], ALPHA, 3, 0)
    st, out = call(gpu, c, x, is_logit, 3, 0)
    assert st == 0 and np.array_equal(out["n_neg"], ref["n_neg"])
    print("loss2", out["loss2"], "oracle", ref["loc_loss"], ref["conf_loss"])
    assert np.isclose(out["loss2"][0], ref["loc_loss"], rtol=1e-5) and np.isclose(out["loss2"][1], ref["conf_loss"], rtol=1e-5)
    assert np.allclose(out["dl"], ref["d_locs"], rtol=1e-4, atol=1e-6)
    assert np.allclose(out["dz"], ref["d_conf_in"], rtol=1e-4, atol=1e-6)
    dropped = (c["match"] < 0) & ~ref["mask"]
    assert np.all(out["dz"].view(np.uint32)[dropped] == 0)
    # grad_scale multiplies the gradients of what is kept; a dropped negative stays +0 whatever its sign
    st, neg = call(gpu, c, x, is_logit, 3, 0, grad_scale=-0.5)
    assert st == 0 and np.array_equal(neg["loss2"], out["loss2"])
    assert np.array_equal(neg["dz"][~dropped], out["dz"][~dropped] * np.float32(-0.5))
    assert np.all(neg["dz"].view(np.uint32)[dropped] == 0)


# ----------------------------------------------------------------------------------- byte-identity with the unmined entry
@pytest.mark.parametrize("B,P,G", [(4, 646, 13), (2, 3199, 100)])
@pytest.mark.parametrize("is_logit", [1, 0])
def test_all_negatives_kept_is_the_unmined_function_byte_for_byte(gpu, B, P, G, is_logit):
    c = make_case(B, P, G)
    x = c["z"] if is_logit else c["x"]
    st_m, mined = call(gpu, c, x, is_logit, 3, P, grad_scale=0.25)
    st_p, plain = call(gpu, c, x, is_logit, mined=False, grad_scale=0.25)
    assert st_m == 0 and st_p == 0
    assert np.array_equal(mined["n_neg"], P - c["n_pos"])
    for k in ("loss2", "dl", "dz"):
        assert mined[k].tobytes() == plain[k].tobytes(), k


# ---------------------------------------------------------------------- the gradients, against float32 numpy: exact
def exact_gradients(c, grad_scale, mask=None):
    """d_logits and d_raw_locs for confidences `x` given as they are (conf_is_logit = 0: no expf), restated in numpy
    float32.  Every step of the kernel is then one correctly rounded float32 operation -- c = x + 1e-10f,
    w = (1 - c) + 1e-10f, (-1 / c) * grad_scale on a positive, (1 / w) * grad_scale on a counted negative,
    (alpha * grad_scale) * (l - g) -- and numpy float32 does the same operations.  mask: the negatives that count (None =
    all); the others get +0."""
    f = np.float32
    pos = c["match"] >= 0
    cc = c["x"] + f(1e-10)
    w = (f(1) - cc) + f(1e-10)
    dz = np.where(pos, (f(-1) / cc) * f(grad_scale), (f(1) / w) * f(grad_scale)).astype(f)
    if mask is not None:
        dz[~pos & ~mask] = f(0)
    dl = np.zeros(c["dec"].shape, f)
    a = f(ALPHA) * f(grad_scale)
    for b in range(c["B"]):
        p = np.nonzero(pos[b])[0]
        dl[b, p] = a * (c["dec"][b, p] - c["gt"][b, c["match"][b, p]])
    assert dz.dtype == f and dl.dtype == f
    return dz, dl


@pytest.mark.parametrize("B,P,G", SHAPES[:3])                 # under one wavefront with an image without negatives; a
@pytest.mark.parametrize("kind", ["plain", "zeros"])          # partial second wavefront; three strides, the last ragged
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("entry", ["plain", "mined", "focal"])
def test_confidence_input_gradients_are_exact(gpu, B, P, G, kind, grad_scale, entry):
    c = make_case(B, P, G, kind)
    mask = MO.select(c["x"], c["match"], 3, 0)[0] if entry == "mined" else None
    kw = dict(plain={}, mined=dict(neg_per_pos=3), focal=dict(gamma=0.0, alpha=None))[entry]
    st, out = LC.call(gpu, c, c["x"], 0, entry=entry, grad_scale=grad_scale, **kw)
    assert st == 0
    dz, dl = exact_gradients(c, grad_scale, mask)
    print("d_logits: %d of %d differ; d_raw_locs: %d of %d differ" % (
        (out["dz"].view(np.uint32) != dz.view(np.uint32)).sum(), dz.size,
        (out["dl"].view(np.uint32) != dl.view(np.uint32)).sum(), dl.size))
    assert out["dz"].tobytes() == dz.tobytes()
    assert out["dl"].tobytes() == dl.tobytes()


# ------------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, B, P, G):
    c = make_case(B, P, G, "quantised")
    _, full = call(gpu, c, c["x"], 0)
    _, again = call(gpu, c, c["x"], 0)
    for k in ("loss2", "dl", "dz", "n_neg"):
        assert full[k].tobytes() == again[k].tobytes(), k
    for b in range(B):
        st, alone = call(gpu, c, c["x"], 0, rows=slice(b, b + 1))
        assert st == 0
        assert alone["dz"].tobytes() == full["dz"][b:b + 1].tobytes() and alone["n_neg"][0] == full["n_neg"][b]
        assert alone["dl"].tobytes() == full["dl"][b:b + 1].tobytes()


# ---------------------------------------------------------------------------------------------------------------- NaN
def test_a_nan_negative_is_taken_first_and_only_where_something_is_taken(gpu):
    c = make_case(4, 70, 5)
    neg1, neg0 = np.nonzero(c["match"][1] < 0)[0], np.nonzero(c["match"][0] < 0)[0]
    z = c["z"].copy()
    z[1, neg1[-1]] = np.nan                                   # image 1: 5 positives, K = 15
    mask, K = MO.select(z, c["match"], 3, 0)
    assert K[1] == 15 and mask[1, neg1[-1]]
    st, out = call(gpu, c, z, 1)
    assert st == 0 and np.array_equal(out["n_neg"], K)
    assert np.isnan(out["dz"][1, neg1[-1]]) and np.isnan(out["loss2"][1]) and np.isfinite(out["loss2"][0])
    assert np.array_equal((out["dz"] != 0) & (c["match"] < 0), mask)
    z = c["z"].copy()
    z[0, neg0[3]] = np.nan                                    # image 0: no positive, K = 0: the NaN is never looked at
    st, out = call(gpu, c, z, 1)
    assert st == 0 and out["n_neg"][0] == 0
    assert np.isfinite(out["loss2"]).all() and not out["dz"][0].any()


# ------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("kw,status", [(dict(neg_per_pos=0), -1), (dict(min_neg=-1), -1), (dict(ws_short=1), -4)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, kw, status):
    c = make_case(4, 70, 5)
    st, out = call(gpu, c, c["z"], 1, prefill=SENTINEL, **kw)
    assert st == status
    assert np.all(out["loss2"] == SENTINEL) and np.all(out["dl"] == SENTINEL) and np.all(out["dz"] == SENTINEL)
    assert np.all(out["n_neg"] == int(SENTINEL))
    st, out = call(gpu, c, c["z"], 1, prefill=SENTINEL)       # the same buffers are written by a good call
    assert st == 0 and not np.any(out["dz"] == SENTINEL) and not np.any(out["n_neg"] == int(SENTINEL))


# ------------------------------------------------------------------------------------------------ through MultiboxLoss
def test_multibox_loss_without_the_switch_is_unchanged(gpu, batch):
    torch, _ = gpu
    from multibox_amd import loss as L
    old = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA)                      # the call as it always was
    new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, neg_per_pos=None, min_neg=0)
    assert new.n_neg is None and new.ws.numel() == old.ws.numel()
    a, b = _forward_backward(torch, old, batch), _forward_backward(torch, new, batch)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # and both are mbx_loss_fwd_bwd on the matcher's output
    c = dict(dec=new.decoded.cpu().numpy(), gt=batch["gt"], match=new.match.cpu().numpy(), P=batch["P"], G=batch["G"])
    _, plain = call(gpu, c, batch["logits"], 1, mined=False)
    assert plain["loss2"].tobytes() == b[0].tobytes() and plain["dz"].tobytes() == b[2].tobytes()


def test_multibox_loss_mined_with_the_real_matcher(gpu, batch):
    torch, _ = gpu
    from multibox_amd import loss as L
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, neg_per_pos=3, min_neg=2)
    loss2, dl, dz = _forward_backward(torch, ml, batch)
    match = ml.match.cpu().numpy()
    assert np.array_equal((match >= 0).sum(1), batch["n"])
    ref = MO.mined_loss(ml.decoded.cpu().numpy(), batch["logits"], 1, batch["gt"], match, ALPHA, 3, 2)
    assert ref["n_neg"].tolist() == [39, 2, 9, 21]
    assert np.array_equal(ml.n_neg.cpu().numpy(), ref["n_neg"])
    assert np.array_equal((dz != 0) & (match < 0), ref["mask"])
    assert np.isclose(loss2[0], ref["loc_loss"], rtol=1e-5) and np.isclose(loss2[1], ref["conf_loss"], rtol=1e-5)
    assert np.allclose(dl, ref["d_locs"], rtol=1e-4, atol=1e-6) and np.allclose(dz, ref["d_conf_in"], rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------------------------------- through the Trainer
def test_trainer_step_mined_graph_equals_eager(gpu):
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
        tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, neg_per_pos=3)
        tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0
        match = tr.loss.match.cpu().numpy()
        n_neg = tr.loss.n_neg.cpu().numpy()
        assert np.array_equal(n_neg, MO.n_selected(match, 3, 0)) and n_neg.tolist() == [9, 0]
        assert tr.mined_negatives_per_image() == 4.5
        # the gradient the backward pass started from: zero on every unselected negative, none on the image without boxes
        dz = net.d_logits.reshape(2, -1).cpu().numpy()
        assert ((dz != 0) & (match < 0)).sum(1).tolist() == [9, 0]
        res.append((tr.loss.loss2.cpu().numpy(), n_neg))
    assert res[0][0].tobytes() == res[1][0].tobytes() and np.isfinite(res[0][0]).all()
    assert np.array_equal(res[0][1], res[1][1])
