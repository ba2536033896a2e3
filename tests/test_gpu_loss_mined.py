"""GPU: mbx_loss_fwd_bwd_mined (hard-negative mining of the confidence loss) against tests/mined_oracle.py.

The C ABI is driven directly with a hand-made `match`, so nothing here depends on the matcher.  Bars: the selection
(which negatives count, n_neg, the +0 gradients of the others) is exact; loss values rtol 1e-5, gradients rtol 1e-4 /
atol 1e-6 (the bars of mbx_loss_fwd_bwd in test_gpu_postproc.py); K = N_neg is byte-identical to mbx_loss_fwd_bwd.
"""
import numpy as np
import pytest

from tests import mined_oracle as MO

pytestmark = pytest.mark.gpu

ALPHA = 1000.0
SHAPES = [(3, 13, 13), (4, 70, 5), (4, 646, 13), (2, 3199, 100)]
SENTINEL = 7.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from multibox_amd import _lib
    return torch, _lib.lib()


def make_case(B, P, G, kind="plain", seed=0):
    """Seeded inputs with a hand-made match: image 0 has no positive, image 1 the most there can be (min(G, P): at
    (3, 13, 13) it has no negative at all), the others a random number.  `x` holds confidences in (0, 1) -- `kind` says
    which -- and `z` logits."""
    rng = np.random.RandomState(1000 * P + B + seed)
    n_pos = rng.randint(1, min(G, P) + 1, B)
    n_pos[0], n_pos[1] = 0, min(G, P)
    match = -np.ones((B, P), np.int32)
    for b in range(B):
        match[b, rng.permutation(P)[:n_pos[b]]] = rng.permutation(G)[:n_pos[b]]
    x = rng.uniform(0.01, 0.99, (B, P)).astype(np.float32)
    if kind == "quantised":                                   # 16 levels: long runs of equal keys
        x = (np.floor(x * 16) / 16).astype(np.float32)
    elif kind == "zeros":                                     # most entries +0.0 or -0.0: one run of equal keys, two bit patterns
        r = rng.uniform(size=(B, P))
        x = np.where(r < 0.4, np.float32(0.0), np.where(r < 0.8, np.float32(-0.0), x)).astype(np.float32)
    return dict(B=B, P=P, G=G, n_pos=n_pos, match=match, x=x, z=(rng.randn(B, P) * 2 - 1).astype(np.float32),
                dec=rng.uniform(0, 1, (B, P, 4)).astype(np.float32), gt=rng.uniform(0, 1, (B, G, 4)).astype(np.float32))


def call(gpu, c, conf_in, is_logit, neg_per_pos=3, min_neg=0, rows=None, grad_scale=1.0, mined=True, ws_short=0,
         prefill=None):
    """One call of the C ABI on images `rows` of case c -> (status, dict of numpy outputs)."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).cuda()
    dec, x, gt, match = dev(c["dec"]), dev(conf_in), dev(c["gt"]), dev(c["match"])
    B, P, G = match.shape[0], c["P"], c["G"]
    fill = (lambda *s, dt=torch.float32: torch.full(s, prefill, dtype=dt, device="cuda")) if prefill is not None else \
        (lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device="cuda"))
    loss2, dl, dz, n_neg = fill(2), fill(B, P, 4), fill(B, P), fill(B, dt=torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    if mined:
        ws = torch.empty((l.mbx_loss_mined_workspace_bytes(B, P),), dtype=torch.uint8, device="cuda")
        st = l.mbx_loss_fwd_bwd_mined(dec.data_ptr(), x.data_ptr(), int(is_logit), gt.data_ptr(), match.data_ptr(), ALPHA,
                                      grad_scale, B, P, G, loss2.data_ptr(), dl.data_ptr(), dz.data_ptr(), neg_per_pos,
                                      min_neg, n_neg.data_ptr(), ws.data_ptr(), ws.numel() - ws_short, s)
    else:
        ws = torch.empty((l.mbx_loss_workspace_bytes(B),), dtype=torch.uint8, device="cuda")
        st = l.mbx_loss_fwd_bwd(dec.data_ptr(), x.data_ptr(), int(is_logit), gt.data_ptr(), match.data_ptr(), ALPHA,
                                grad_scale, B, P, G, loss2.data_ptr(), dl.data_ptr(), dz.data_ptr(), ws.data_ptr(),
                                ws.numel(), s)
    torch.cuda.synchronize()
    return st, dict(loss2=loss2.cpu().numpy(), dl=dl.cpu().numpy(), dz=dz.cpu().numpy(), n_neg=n_neg.cpu().numpy())


def check_selection(c, out, mask, K):
    """With conf_is_logit = 0 a selected negative's gradient is 1/w != 0, so d_logits shows the selection."""
    neg = c["match"] < 0
    assert np.array_equal(out["n_neg"], K)
    assert np.array_equal((out["dz"] != 0) & neg, mask)
    assert np.all(out["dz"].view(np.uint32)[neg & ~mask] == 0)            # +0.0f by bits
    assert np.all(out["dz"][~neg] < 0)                                    # positives: -1/c


def cut_splits_a_run(c, mask):
    """Images in which negatives with bit-equal keys lie on both sides of the cut."""
    key = MO.score_order_key(c["x"])
    hit = []
    for b in range(c["B"]):
        neg = c["match"][b] < 0
        if np.intersect1d(key[b][neg & mask[b]], key[b][neg & ~mask[b]]).size:
            hit.append(b)
    return hit


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
@pytest.fixture(scope="module")
def batch():
    """Raw network outputs and ground truth for MultiboxLoss at P = 646, B = 4 (image 1 without boxes)."""
    from multibox_amd import priors as PR
    priors = np.array(PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.]), np.float32)
    rng = np.random.RandomState(5)
    B, P, G = 4, priors.shape[0], 13
    raw = (rng.randn(B, P, 4) * 0.05).astype(np.float32)
    logits = (rng.randn(B, P) * 2 - 2).astype(np.float32)
    n = np.array([G, 0, 3, 7], np.int32)
    gt = np.zeros((B, G, 4), np.float32)
    for b in range(B):
        xy = rng.uniform(0, .7, (n[b], 2)); wh = rng.uniform(.05, .3, (n[b], 2))
        gt[b, :n[b], :2] = xy; gt[b, :n[b], 2:] = xy + wh
    return dict(priors=priors, raw=raw, logits=logits, gt=gt, n=n, B=B, P=P, G=G)


def _forward_backward(torch, ml, batch):
    out = ml.forward_backward(torch.from_numpy(batch["raw"]).cuda(), torch.from_numpy(batch["logits"]).cuda(),
                              torch.from_numpy(batch["gt"]).cuda(), torch.from_numpy(batch["n"]).cuda())
    torch.cuda.synchronize()
    assert int(ml.status.max()) == 0
    return [t.cpu().numpy() for t in out]


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
