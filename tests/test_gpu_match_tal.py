"""GPU: mbx_match_tal (task-aligned matching behind the bipartite match) against tests/tal_oracle.py.

The C ABI is driven directly with a hand-made `match`, so the first half depends on no matcher.  The bar is exactness: the
kernel's float64 arithmetic has the oracle's operations in the oracle's order, so `match`, `n_extra` and `thr` are compared
byte for byte.  The cases (tests/tal_cases.py; tests/test_tal_cpu.py asserts what each of them exercises): fewer priors than
one wavefront (13), P no multiple of 64 (70), the same on a 1/64 lattice with equal metrics on both sides of the cut, topk 1,
topk over every candidate (no round runs), the square-root branch, t = u, the real priors at 299 px (646) and at 512 px
(3 199, G = 100: boxes in a row on each wavefront), and 300 of 646 candidates taken, which makes the wavefront scan again.
"""
import numpy as np
import pytest

from tests import tal_cases as TC
from tests import tal_oracle as TO
from tests import ignore_oracle as IO
from tests import mined_oracle as MO
from tests import loss_cases as LC
from tests.loss_cases import ALPHA, batch, gpu  # noqa: F401  (the fixtures are found by name)

pytestmark = pytest.mark.gpu

SENTINEL = -77
THR_SENTINEL = -7.5


def call(gpu, c, rows=None, with_extra=True, with_thr=True, null=None, topk=None, halves=None, beta=None, **override):
    """One call of the C ABI on images `rows` of case c (arrays in `override` replace the case's) ->
    (status, match [B,P], n_extra [B] prefilled with SENTINEL, thr [B,G] prefilled with THR_SENTINEL)."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    get = lambda k: override.get(k, c[k])
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()                 # a copy: the case's arrays are read-only
    priors, decoded, conf, gt = dev(get("priors")), dev(get("decoded")[rows]), dev(get("conf")[rows]), dev(get("gt")[rows])
    n, status, match = dev(get("n")[rows]), dev(get("status")[rows]), dev(get("match")[rows])
    B, P = match.shape
    n_extra = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    thr = torch.full((B, c["G"]), THR_SENTINEL, dtype=torch.float64, device="cuda")
    ptr = lambda name, t: None if null == name else t.data_ptr()
    st = l.mbx_match_tal(ptr("priors", priors), ptr("decoded", decoded), ptr("conf", conf), ptr("gt", gt), ptr("n_gt", n),
                         ptr("status", status), c["topk"] if topk is None else topk,
                         TO.alpha_halves(c["alpha"]) if halves is None else halves, c["beta"] if beta is None else beta,
                         override.get("B", B), override.get("P", P), override.get("G", c["G"]), ptr("match", match),
                         n_extra.data_ptr() if with_extra else None, thr.data_ptr() if with_thr else None,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, match.cpu().numpy(), n_extra.cpu().numpy(), thr.cpu().numpy()


# --------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", list(TC.CASES))
def test_match_n_extra_and_thr_equal_the_oracle(gpu, name):
    c = TC.make_case(name)
    want, want_extra, want_thr = TC.oracle(name)
    assert want_extra.sum() >= 1 and want_extra[0] == 0                   # the case adds something, or it shows nothing
    st, match, n_extra, thr = call(gpu, c)
    print("added per image", n_extra, "oracle", want_extra)
    assert st == 0
    assert thr.tobytes() == want_thr.tobytes()
    assert match.tobytes() == want.tobytes() and n_extra.tobytes() == want_extra.tobytes()
    had = c["match"] >= 0
    assert np.array_equal(match[had], c["match"][had])                    # what was matched keeps its box


def test_by_hand(gpu):
    quad = np.array([[0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1], [.5, .5, 1, 1]], np.float32)
    c = dict(B=1, P=4, G=1, topk=1, alpha=1.5, beta=3, priors=quad, decoded=quad[None], conf=np.full((1, 4), .5, np.float32),
             gt=np.array([[[0, 0, .5, .375]]], np.float32), n=np.array([1], np.int32), status=np.zeros(1, np.int32),
             match=-np.ones((1, 4), np.int32))
    st, match, n_extra, thr = call(gpu, c)
    assert st == 0 and thr.tolist() == [[(0.5 * np.sqrt(0.5)) * (0.75 * 0.75 * 0.75)]]
    assert match.tolist() == [[0, -1, -1, -1]] and n_extra.tolist() == [1]
    on_edge = dict(c, gt=np.array([[[0, 0, .5, .25]]], np.float32))       # y2 == the prior's cy: not inside
    st, match, n_extra, thr = call(gpu, on_edge)
    assert st == 0 and thr.tolist() == [[0.0]] and match.tolist() == [[-1] * 4] and n_extra.tolist() == [0]
    same = np.tile(np.array([[.25, .25, .75, .75]], np.float32), (4, 1))  # four priors, one prediction: equal t
    pred = np.tile(np.array([[.25, .25, .75, .625]], np.float32), (1, 4, 1))
    tied = dict(c, priors=same, decoded=pred, gt=np.array([[[.25, .25, .75, .75]]], np.float32), topk=2, alpha=1.0, beta=1)
    st, match, n_extra, thr = call(gpu, tied)
    assert st == 0 and thr.tolist() == [[0.375]] and match.tolist() == [[0, 0, -1, -1]] and n_extra.tolist() == [2]


def test_a_nan_prediction_is_never_selected(gpu):
    c = TC.make_case("p70")
    full, _, _ = TC.oracle("p70")
    hit = np.argwhere((full >= 0) & (c["match"] < 0))[:8]
    decoded, conf = c["decoded"].copy(), c["conf"].copy()
    for i, (b, p) in enumerate(hit[:4]):
        decoded[b, p, i] = np.nan
    for b, p in hit[4:6]:
        decoded[b, p] = np.nan
    for b, p in hit[6:8]:
        conf[b, p] = np.nan
    want = TO.tal(c["priors"], decoded, conf, c["gt"], c["n"], c["status"], c["match"], c["topk"], c["alpha"], c["beta"])
    st, match, n_extra, thr = call(gpu, c, decoded=decoded, conf=conf)
    assert st == 0 and all(match[b, p] == -1 for b, p in hit)
    assert match.tobytes() == want[0].tobytes() and n_extra.tobytes() == want[1].tobytes() and thr.tobytes() == want[2].tobytes()


# ------------------------------------------------------------------------------------- independence and reproducibility
@pytest.mark.parametrize("name", ["p70", "p646", "p3199"])
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, name):
    c = TC.make_case(name)
    _, full, full_extra, full_thr = call(gpu, c)
    _, again, again_extra, again_thr = call(gpu, c)
    assert full.tobytes() == again.tobytes() and full_extra.tobytes() == again_extra.tobytes()
    assert full_thr.tobytes() == again_thr.tobytes()
    perm = np.arange(c["B"])[::-1].copy()
    st, out, extra, thr = call(gpu, c, rows=perm)
    assert st == 0 and out.tobytes() == full[perm].tobytes() and np.array_equal(extra, full_extra[perm])
    assert thr.tobytes() == full_thr[perm].tobytes()
    b = c["B"] - 1                                                        # the fullest image alone
    st, out, extra, thr = call(gpu, c, rows=slice(b, b + 1))
    assert st == 0 and out.tobytes() == full[b:b + 1].tobytes() and extra[0] == full_extra[b]
    assert thr.tobytes() == full_thr[b:b + 1].tobytes()


@pytest.mark.parametrize("name", ["p70", "p646"])
def test_every_output_element_is_written_and_null_outputs_are_accepted(gpu, name):
    c = TC.make_case(name)
    want, want_extra, want_thr = TC.oracle(name)
    st, match, n_extra, thr = call(gpu, c)                                # prefilled with the sentinels
    assert st == 0 and not np.any(n_extra == SENTINEL) and not np.any(thr == THR_SENTINEL)
    st, match, n_extra, thr = call(gpu, c, with_extra=False)
    assert st == 0 and match.tobytes() == want.tobytes() and np.all(n_extra == SENTINEL) and thr.tobytes() == want_thr.tobytes()
    st, match, n_extra, thr = call(gpu, c, with_thr=False)
    assert st == 0 and match.tobytes() == want.tobytes() and np.all(thr == THR_SENTINEL)
    assert n_extra.tobytes() == want_extra.tobytes()
    st, match, n_extra, thr = call(gpu, c, with_extra=False, with_thr=False)
    assert st == 0 and match.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------- what stays untouched
@pytest.mark.parametrize("name", ["p13", "p70", "p646"])
def test_skipped_images_keep_their_row_byte_for_byte(gpu, name):
    c = TC.make_case(name)
    B, P = c["B"], c["P"]
    want, want_extra, want_thr = TC.oracle(name)
    pattern = (np.arange(B * P, dtype=np.int32).reshape(B, P) % 5) - 3     # -3 .. 1: free and "matched" entries alike
    for bad in (1, 2):
        status = np.zeros(B, np.int32)
        status[1] = bad
        match = c["match"].copy()
        match[1] = pattern[1]
        st, out, n_extra, thr = call(gpu, c, status=status, match=match)
        assert st == 0
        assert out[1].tobytes() == pattern[1].tobytes() and n_extra[1] == 0 and not thr[1].any()
        assert out[0].tobytes() == c["match"][0].tobytes() and n_extra[0] == 0 and not thr[0].any()      # n_gt = 0
        keep = [b for b in range(B) if b != 1]
        assert out[keep].tobytes() == want[keep].tobytes() and np.array_equal(n_extra[keep], want_extra[keep])
        assert thr[keep].tobytes() == want_thr[keep].tobytes()
    n = c["n"].copy()
    n[1] = c["G"] + 1                                                     # more boxes than rows: skipped, nothing read
    match = c["match"].copy()
    match[1] = pattern[1]
    st, out, n_extra, thr = call(gpu, c, n=n, match=match)
    assert st == 0 and out[1].tobytes() == pattern[1].tobytes() and n_extra[1] == 0 and not thr[1].any()


@pytest.mark.parametrize("name", ["p70", "p646"])
def test_a_nan_in_the_padding_rows_changes_nothing(gpu, name):
    c = TC.make_case(name)
    want, want_extra, want_thr = TC.oracle(name)
    gt = c["gt"].copy()
    for b in range(c["B"]):
        gt[b, c["n"][b]:] = np.nan
    assert np.isnan(gt).any()
    st, match, n_extra, thr = call(gpu, c, gt=gt)
    assert st == 0 and match.tobytes() == want.tobytes() and n_extra.tobytes() == want_extra.tobytes()
    assert thr.tobytes() == want_thr.tobytes()


# --------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("kw", [dict(null="priors"), dict(null="decoded"), dict(null="conf"), dict(null="gt"), dict(null="n_gt"),
                                dict(null="status"), dict(null="match"), dict(B=-1), dict(P=0), dict(G=0), dict(topk=0),
                                dict(halves=-1), dict(halves=9), dict(beta=0), dict(beta=17)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, kw):
    c = TC.make_case("p70")
    sentinel = np.full((4, 70), SENTINEL, np.int32)
    st, match, n_extra, thr = call(gpu, c, match=sentinel, **kw)
    assert st == -1
    assert np.all(match == SENTINEL) and np.all(n_extra == SENTINEL) and np.all(thr == THR_SENTINEL)


def test_an_unsupported_size_is_refused_and_nothing_is_written(gpu):
    torch, l = gpu
    c = TC.make_case("p70")
    sentinel = np.full((4, 70), SENTINEL, np.int32)
    # G is refused before any pointer is followed: nothing is launched, so the small buffers are never indexed
    st, match, n_extra, thr = call(gpu, c, match=sentinel, G=1 << 20)
    assert st == -2 and l.mbx_match_tal_supported(70, 1 << 20, 4) == -2
    assert np.all(match == SENTINEL) and np.all(n_extra == SENTINEL) and np.all(thr == THR_SENTINEL)
    st, match, n_extra, thr = call(gpu, c)                                 # the same call with the real G writes
    assert st == 0 and not np.any(n_extra == SENTINEL)
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    f = torch.zeros(8, dtype=torch.float32, device="cuda")
    assert l.mbx_match_tal(f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), z.data_ptr(), z.data_ptr(), 13, 2, 6, 0, 1, 1,
                           z.data_ptr(), None, None, None) == 0            # B == 0


# ------------------------------------------------------------------------------------------------ through MultiboxLoss
TOPK = 13


def _forward_backward(torch, ml, batch):
    """loss_cases' three outputs and the match they were computed on."""
    return LC._forward_backward(torch, ml, batch) + [ml.match.cpu().numpy()]


@pytest.fixture(scope="module")
def plain(gpu, batch):
    """MultiboxLoss as it always was called, on the batch: (loss2, d_locs, d_logits, match) and the decoded predictions and
    confidences the match read."""
    from multibox_amd import loss as L
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA)
    return _forward_backward(gpu[0], ml, batch) + [ml.decoded.cpu().numpy(), ml.conf.cpu().numpy()]


@pytest.fixture(scope="module")
def selected(batch, plain):
    """The oracle at topk 13, alpha 1, beta 6 on the bipartite match of `plain`: (match, n_extra, thr)."""
    return TO.tal(batch["priors"], plain[4], plain[5], batch["gt"], batch["n"], np.zeros(batch["B"], np.int32), plain[3], TOPK)


def test_multibox_loss_without_the_key_is_unchanged(gpu, batch, plain):
    torch, _ = gpu
    from multibox_amd import loss as L
    new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, tal_topk=None, tal_alpha=1.0, tal_beta=6)
    assert new.n_tal is None and new.tal_thr is None
    for x, y in zip(plain[:4], _forward_backward(torch, new, batch)):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal((plain[3] >= 0).sum(1), batch["n"])             # bipartite: one prior per box


def _direct(gpu, batch, ml, entry, match, ws_bytes, *args):
    """The loss entry called directly on `match` with the decoded predictions ml left -> (loss2, d_locs, d_logits) numpy."""
    torch, l = gpu
    B, P, G = batch["B"], batch["P"], batch["G"]
    f = dict(dtype=torch.float32, device="cuda")
    d_loss2, d_dl, d_dz = torch.zeros(2, **f), torch.zeros(B, P, 4, **f), torch.zeros(B, P, **f)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    logits, gt, m = torch.from_numpy(batch["logits"]).cuda(), torch.from_numpy(batch["gt"]).cuda(), torch.from_numpy(match).cuda()
    st = getattr(l, entry)(ml.decoded.data_ptr(), logits.data_ptr(), 1, gt.data_ptr(), m.data_ptr(), ALPHA, 1.0, B, P, G,
                           d_loss2.data_ptr(), d_dl.data_ptr(), d_dz.data_ptr(), *args, ws.data_ptr(), ws.numel(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    return d_loss2.cpu().numpy(), d_dl.cpu().numpy(), d_dz.cpu().numpy()


def test_multibox_loss_with_the_key(gpu, batch, plain, selected):
    torch, l = gpu
    from multibox_amd import loss as L
    want, want_extra, want_thr = selected
    assert want_extra.sum() >= 1 and want_extra[1] == 0
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, tal_topk=TOPK)
    loss2, dl, dz, match = _forward_backward(torch, ml, batch)
    print("added per image", ml.n_tal.tolist(), "location loss", plain[0][0], "->", loss2[0])
    assert match.tobytes() == want.tobytes() and np.array_equal(ml.n_tal.cpu().numpy(), want_extra)
    assert ml.tal_thr.cpu().numpy().tobytes() == want_thr.tobytes()
    # the loss is mbx_loss_fwd_bwd on the extended match: the same entry point, called directly
    d_loss2, d_dl, d_dz = _direct(gpu, batch, ml, "mbx_loss_fwd_bwd", want, l.mbx_loss_workspace_bytes(batch["B"]))
    assert loss2.tobytes() == d_loss2.tobytes() and dl.tobytes() == d_dl.tobytes() and dz.tobytes() == d_dz.tobytes()
    assert loss2[0] > plain[0][0]                                         # more positives: a strictly larger location loss


def test_multibox_loss_with_the_key_and_mining(gpu, batch, selected):
    torch, _ = gpu
    from multibox_amd import loss as L
    want, want_extra, _ = selected
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, neg_per_pos=3, tal_topk=TOPK)
    _, _, _, match = _forward_backward(torch, ml, batch)
    assert match.tobytes() == want.tobytes()
    n_neg = ml.n_neg.cpu().numpy()
    assert np.array_equal(n_neg, MO.n_selected(want, 3, 0))
    assert np.array_equal(n_neg, 3 * (batch["n"] + want_extra))           # the budget grew with the added positives
    assert np.array_equal(n_neg, 3 * (batch["n"] + ml.n_tal.cpu().numpy()))


def test_multibox_loss_with_the_key_varifocal_giou_and_the_ignore_band(gpu, batch, plain, selected):
    torch, l = gpu
    from multibox_amd import loss as L
    want, _, _ = selected
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, tal_topk=TOPK, quality_target="varifocal", loc_loss="giou",
                        ignore_iou_threshold=0.4, ignore_source="prediction")
    loss2, dl, dz, match = _forward_backward(torch, ml, batch)
    # the band runs behind the task-aligned launch, on the same decoded predictions
    banded, n_ignored = IO.ignore(plain[4], 1, batch["gt"], batch["n"], np.zeros(batch["B"], np.int32), want, 0.4)
    assert match.tobytes() == banded.tobytes() and np.array_equal(ml.n_ignored.cpu().numpy(), n_ignored)
    assert n_ignored.sum() >= 1 and np.array_equal(match[match >= 0], want[match >= 0]) and np.array_equal(match >= 0, want >= 0)
    q_stats = torch.zeros((batch["B"], 2), dtype=torch.float64, device="cuda")
    d_loss2, d_dl, d_dz = _direct(gpu, batch, ml, "mbx_loss_fwd_bwd_ignore", match,
                                  l.mbx_loss_ignore_workspace_bytes(batch["B"], batch["P"]), L.LOC_TYPES.index("giou"), 0.0, 2, 2.0,
                                  1.0, 0.75, 0, 0, None, q_stats.data_ptr())
    assert np.isfinite(loss2).all()
    assert loss2.tobytes() == d_loss2.tobytes() and dl.tobytes() == d_dl.tobytes() and dz.tobytes() == d_dz.tobytes()
    assert ml.q_stats.cpu().numpy().tobytes() == q_stats.cpu().numpy().tobytes()


def test_tal_matches_wrapper(gpu, batch, plain, selected):
    torch, _ = gpu
    from multibox_amd import loss as L, _lib
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, G = batch["B"], batch["G"]
    match, n_extra = dev(plain[3]), torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    thr = torch.full((B, G), THR_SENTINEL, dtype=torch.float64, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    args = (dev(batch["priors"]), dev(plain[4]), dev(plain[5]), dev(batch["gt"]), dev(batch["n"]), status, match)
    out, extra, t = L.tal_matches(*args, TOPK, n_extra=n_extra, thr=thr)
    torch.cuda.synchronize()
    assert out is match and extra is n_extra and t is thr
    assert match.cpu().numpy().tobytes() == selected[0].tobytes() and np.array_equal(n_extra.cpu().numpy(), selected[1])
    assert thr.cpu().numpy().tobytes() == selected[2].tobytes()
    # other exponents through the wrapper
    match2 = dev(plain[3])
    L.tal_matches(*args[:6], match2, 5, alpha=0.5, beta=2)
    torch.cuda.synchronize()
    want = TO.tal(batch["priors"], plain[4], plain[5], batch["gt"], batch["n"], np.zeros(B, np.int32), plain[3], 5, 0.5, 2)[0]
    assert match2.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(_lib.MbxError):
        L.tal_matches(*args, 0)
    with pytest.raises(ValueError):
        L.tal_matches(*args, TOPK, alpha=0.3)


# ---------------------------------------------------------------------------------------------------- through the Trainer
def _trainer_step(torch, use_graph):
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer
    from multibox_amd import priors as PR, loss as L
    priors = np.array(PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.]), np.float32)
    gen = torch.Generator().manual_seed(3)
    images = torch.rand(2, 299, 299, 3, generator=gen) * 2 - 1
    rng = np.random.RandomState(1)
    n_gt = np.array([3, 0], np.int32)
    gt = np.zeros((2, 13, 4), np.float32)
    xy = rng.uniform(0, .7, (3, 2)); wh = rng.uniform(.05, .3, (3, 2))
    gt[0, :3, :2] = xy; gt[0, :3, 2:] = xy + wh
    net = Net(batch=2, input_size=299, k=5, mode="train", seed=5)
    tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, tal_topk=TOPK)
    tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
    tr.step()
    torch.cuda.synchronize()
    assert int(tr.match_status().max()) == 0
    match = tr.loss.match.cpu().numpy()
    n_tal = tr.loss.n_tal.cpu().numpy()
    # the bipartite part: mbx_match again on the decoded locations and confidences the step left behind
    bip, st = L.match_boxes(tr.loss.decoded, tr.loss.conf, tr.gt, tr.n_gt, tr.loss.alpha)
    torch.cuda.synchronize()
    bip = bip.cpu().numpy()
    assert int(st.max()) == 0 and (bip >= 0).sum(1).tolist() == [3, 0]
    want, want_extra, want_thr = TO.tal(priors, tr.loss.decoded.cpu().numpy(), tr.loss.conf.cpu().numpy(), gt, n_gt,
                                        np.zeros(2, np.int32), bip, TOPK)
    print("added per image", n_tal)
    assert match.tobytes() == want.tobytes() and np.array_equal(n_tal, want_extra)
    assert tr.loss.tal_thr.cpu().numpy().tobytes() == want_thr.tobytes()
    assert n_tal[1] == 0
    assert tr.tal_matches_per_image() == float(n_tal.mean()) and tr.atss_matches_per_image() is None
    return tr, net, priors, (tr.loss.loss2.cpu().numpy(), match, n_tal)


def test_trainer_step_with_tal_graph_equals_eager(gpu):
    torch, _ = gpu
    from multibox_amd.trainer import Trainer
    res = []
    for use_graph in (True, False):
        tr, net, priors, out = _trainer_step(torch, use_graph)
        res.append(out)
    assert res[0][0].tobytes() == res[1][0].tobytes() and np.isfinite(res[0][0]).all()
    assert res[0][1].tobytes() == res[1][1].tobytes() and np.array_equal(res[0][2], res[1][2])
    # without the key: nothing to report (a second trainer on the last net; it is built, never stepped)
    assert Trainer(net, priors, max_num_bboxes=13, use_graph=False).tal_matches_per_image() is None
    # a fresh network's predictions may overlap nothing inside the boxes (here they add a few): the same loss object on
    # predictions that sit on the priors (raw locations 0) and the step's own scores has to add something
    raw = torch.zeros((2, net.P, 4), dtype=torch.float32, device="cuda")
    logits = torch.logit((tr.loss.conf - 1e-10).clamp(1e-6, 1 - 1e-6)).contiguous()
    tr.loss.forward_backward(raw, logits, tr.gt, tr.n_gt)
    torch.cuda.synchronize()
    n_tal = tr.loss.n_tal.cpu().numpy()
    print("added per image with the predictions on the priors", n_tal)
    assert int(tr.loss.status.max()) == 0 and n_tal[0] > 0 and n_tal[1] == 0
