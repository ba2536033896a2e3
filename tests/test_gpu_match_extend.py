"""GPU: mbx_match_extend (threshold matching behind the bipartite match) against tests/extend_oracle.py.

The C ABI is driven directly with a hand-made `match`, so the first half depends on no matcher.  The bar is exactness:
the kernel's float64 IoU has the oracle's operations in the oracle's order, so `match` and `n_extra` are compared bit for
bit.  Shapes: fewer priors than one wavefront (13), a partial second wavefront (70), eleven wavefronts of which the last is
partial (646), and the strided loop of 1 024 threads with a tail (3 199).
"""
import functools

import numpy as np
import pytest

from tests import extend_oracle as EO
from tests import loss_cases as LC
from tests import mined_oracle as MO
from tests.loss_cases import ALPHA, batch, gpu  # noqa: F401  (the fixtures are found by name)

pytestmark = pytest.mark.gpu

SHAPES = [(3, 13, 13), (4, 70, 5), (4, 646, 13), (2, 3199, 100)]
SENTINEL = -77


@functools.lru_cache(maxsize=None)
def make_case(B, P, G, grid=0):
    """Seeded inputs: random priors, boxes that are jittered copies of random priors (so that some IoUs clear 0.5), a
    hand-made match with a random subset of the priors already matched to distinct boxes.  Image 0 has no box, image 1
    min(G, P) of them.  grid: every coordinate snapped to multiples of 1/grid, and in image 1 boxes 0 and 1 are the
    widest free prior moved one grid step to the right and to the left, so that two boxes have exactly equal IoUs with a
    prior (the arithmetic on multiples of 1/16 is exact).  The arrays are shared between tests: nobody writes to them."""
    rng = np.random.RandomState(1000 * P + B + grid)
    c = rng.uniform(0.1, 0.9, (P, 2)); wh = rng.uniform(0.05, 0.4, (P, 2))
    priors = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    n = rng.randint(1, min(G, P) + 1, B)
    n[0], n[1] = 0, min(G, P)
    gt = np.zeros((B, G, 4), np.float32)
    match = -np.ones((B, P), np.int32)
    for b in range(B):
        gt[b, :n[b]] = priors[rng.randint(0, P, n[b])] + rng.uniform(-0.02, 0.02, (n[b], 4)).astype(np.float32)
        k = rng.randint(0, n[b] + 1) if b != 1 else n[b] // 2
        match[b, rng.permutation(P)[:k]] = rng.permutation(n[b])[:k]
    if grid:
        priors = (np.round(priors * grid) / grid).astype(np.float32)
        gt = (np.round(gt * grid) / grid).astype(np.float32)
        free = np.nonzero(match[1] < 0)[0]
        widest = priors[free[np.argmax(priors[free, 2] - priors[free, 0])]]
        step = np.array([1.0 / grid, 0, 1.0 / grid, 0], np.float32)
        gt[1, 0], gt[1, 1] = widest + step, widest - step
    c = dict(B=B, P=P, G=G, priors=priors, gt=gt, n=n.astype(np.int32), status=np.zeros(B, np.int32), match=match)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle(B, P, G, thr, grid=0):
    c = make_case(B, P, G, grid)
    out, extra = EO.extend(c["priors"], c["gt"], c["n"], c["status"], c["match"], thr)
    out.setflags(write=False); extra.setflags(write=False)
    return out, extra


def call(gpu, c, thr, rows=None, with_extra=True, null_priors=False, **override):
    """One call of the C ABI on images `rows` of case c (arrays in `override` replace the case's) ->
    (status, match [B,P], n_extra [B] prefilled with SENTINEL)."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    get = lambda k: override.get(k, c[k])
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()                 # a copy: the case's arrays are read-only
    priors, gt, n, status, match = dev(get("priors")), dev(get("gt")[rows]), dev(get("n")[rows]), dev(get("status")[rows]), \
        dev(get("match")[rows])
    B, P = match.shape
    n_extra = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    st = l.mbx_match_extend(None if null_priors else priors.data_ptr(), gt.data_ptr(), n.data_ptr(), status.data_ptr(),
                            float(thr), B, P, c["G"], match.data_ptr(), n_extra.data_ptr() if with_extra else None,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, match.cpu().numpy(), n_extra.cpu().numpy()


# --------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("thr", [0.3, 0.5])
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_match_and_n_extra_equal_the_oracle(gpu, B, P, G, thr):
    c = make_case(B, P, G)
    want, want_extra = oracle(B, P, G, thr)
    assert want_extra.sum() >= 1 and want_extra[0] == 0                   # the case adds something, or it shows nothing
    st, match, n_extra = call(gpu, c, thr)
    print("added per image", n_extra, "oracle", want_extra)
    assert st == 0
    assert match.tobytes() == want.tobytes() and n_extra.tobytes() == want_extra.tobytes()
    had = c["match"] >= 0
    assert np.array_equal(match[had], c["match"][had])                    # what was matched keeps its box


def _rows_with_equal_best(c, want):
    """(b, p) of added priors whose largest IoU is reached by two boxes."""
    hit = []
    for b, p in zip(*np.nonzero((want >= 0) & (c["match"] < 0))):
        iou = EO.iou_row(c["priors"][p], c["gt"][b, :c["n"][b]])
        if (iou == iou.max()).sum() > 1:
            hit.append((b, p))
    return hit


@pytest.mark.parametrize("B,P,G", SHAPES)
def test_quantised_coordinates_equal_ious_go_to_the_lowest_index(gpu, B, P, G):
    c = make_case(B, P, G, grid=16)
    want, want_extra = oracle(B, P, G, 0.3, grid=16)
    ties = _rows_with_equal_best(c, want)
    assert ties, "no prior has two equally good boxes: the case shows nothing"
    st, match, n_extra = call(gpu, c, 0.3)
    assert st == 0 and match.tobytes() == want.tobytes() and n_extra.tobytes() == want_extra.tobytes()
    for b, p in ties:
        iou = EO.iou_row(c["priors"][p], c["gt"][b, :c["n"][b]])
        assert match[b, p] == np.nonzero(iou == iou.max())[0][0]


def test_an_iou_of_exactly_the_threshold_is_not_over_it(gpu):
    c = dict(B=1, P=1, G=1, priors=np.array([[0, 0, .5, .5]], np.float32), gt=np.array([[[0, 0, .5, .25]]], np.float32),
             n=np.array([1], np.int32), status=np.zeros(1, np.int32), match=-np.ones((1, 1), np.int32))
    assert EO.iou_row(c["priors"][0], c["gt"][0])[0] == 0.5
    st, match, n_extra = call(gpu, c, 0.5)
    assert st == 0 and match.tolist() == [[-1]] and n_extra.tolist() == [0]
    st, match, n_extra = call(gpu, c, np.nextafter(np.float32(0.5), np.float32(0)))
    assert st == 0 and match.tolist() == [[0]] and n_extra.tolist() == [1]


# ------------------------------------------------------------------------------------------------- what stays untouched
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_skipped_images_keep_their_row_byte_for_byte(gpu, B, P, G):
    c = make_case(B, P, G)
    want, want_extra = oracle(B, P, G, 0.3)
    pattern = (np.arange(B * P, dtype=np.int32).reshape(B, P) % 5) - 3     # -3 .. 1: free and "matched" entries alike
    for bad in (1, 2):
        status = np.zeros(B, np.int32)
        status[1] = bad
        match = c["match"].copy()
        match[1] = pattern[1]
        st, out, n_extra = call(gpu, c, 0.3, status=status, match=match)
        assert st == 0
        assert out[1].tobytes() == pattern[1].tobytes() and n_extra[1] == 0
        assert out[0].tobytes() == c["match"][0].tobytes() and n_extra[0] == 0         # n_gt = 0
        keep = [b for b in range(B) if b != 1]
        assert out[keep].tobytes() == want[keep].tobytes() and np.array_equal(n_extra[keep], want_extra[keep])


@pytest.mark.parametrize("B,P,G", SHAPES)
def test_a_nan_in_the_padding_rows_changes_nothing(gpu, B, P, G):
    c = make_case(B, P, G)
    want, want_extra = oracle(B, P, G, 0.3)
    gt = c["gt"].copy()
    for b in range(B):
        gt[b, c["n"][b]:] = np.nan
    assert np.isnan(gt).any()
    st, match, n_extra = call(gpu, c, 0.3, gt=gt)
    assert st == 0 and match.tobytes() == want.tobytes() and n_extra.tobytes() == want_extra.tobytes()


@pytest.mark.parametrize("B,P,G", SHAPES)
def test_threshold_one_adds_nothing(gpu, B, P, G):
    c = make_case(B, P, G)
    gt = c["gt"].copy()
    gt[1, 0] = c["priors"][np.nonzero(c["match"][1] < 0)[0][0]]           # an IoU of exactly 1 with a free prior
    st, match, n_extra = call(gpu, c, 1.0, gt=gt)
    assert st == 0 and match.tobytes() == c["match"].tobytes() and not n_extra.any()


# ------------------------------------------------------------------------------------- independence and reproducibility
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, B, P, G):
    c = make_case(B, P, G)
    _, full, full_extra = call(gpu, c, 0.3)
    _, again, again_extra = call(gpu, c, 0.3)
    assert full.tobytes() == again.tobytes() and full_extra.tobytes() == again_extra.tobytes()
    st, no_extra, untouched = call(gpu, c, 0.3, with_extra=False)         # n_extra = NULL
    assert st == 0 and no_extra.tobytes() == full.tobytes() and np.all(untouched == SENTINEL)
    perm = np.arange(B)[::-1].copy()
    st, out, extra = call(gpu, c, 0.3, rows=perm)
    assert st == 0 and out.tobytes() == full[perm].tobytes() and np.array_equal(extra, full_extra[perm])
    for b in range(B):
        st, out, extra = call(gpu, c, 0.3, rows=slice(b, b + 1))
        assert st == 0 and out.tobytes() == full[b:b + 1].tobytes() and extra[0] == full_extra[b]


# --------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("kw", [dict(thr=0.0), dict(thr=-0.1), dict(thr=1.5), dict(thr=float("nan")),
                                dict(thr=0.3, null_priors=True)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, kw):
    c = make_case(4, 70, 5)
    sentinel = np.full((4, 70), SENTINEL, np.int32)
    st, match, n_extra = call(gpu, c, match=sentinel, **kw)
    assert st == -1
    assert np.all(match == SENTINEL) and np.all(n_extra == SENTINEL)
    st, match, n_extra = call(gpu, c, 0.3)                                 # the same call with good arguments writes
    assert st == 0 and not np.any(n_extra == SENTINEL)


def test_more_boxes_than_the_lds_holds_is_unsupported(gpu):
    torch, l = gpu
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    f = torch.zeros(8, dtype=torch.float32, device="cuda")
    n_extra = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    # G is refused before any pointer is followed: nothing is launched, so the small buffers are never indexed
    st = l.mbx_match_extend(f.data_ptr(), f.data_ptr(), z.data_ptr(), z.data_ptr(), 0.5, 1, 1, 1 << 20, z.data_ptr(),
                            n_extra.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == -2 and int(n_extra[0]) == SENTINEL
    assert l.mbx_match_extend(f.data_ptr(), f.data_ptr(), z.data_ptr(), z.data_ptr(), 0.5, 0, 1, 1, z.data_ptr(), None, None) == 0


# ------------------------------------------------------------------------------------------------ through MultiboxLoss
def _forward_backward(torch, ml, batch):
    """loss_cases' three outputs and the match they were computed on."""
    return LC._forward_backward(torch, ml, batch) + [ml.match.cpu().numpy()]


@pytest.fixture(scope="module")
def plain(gpu, batch):
    """MultiboxLoss as it always was called, on the batch: (loss2, d_locs, d_logits, match)."""
    from multibox_amd import loss as L
    return _forward_backward(gpu[0], L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA), batch)


@pytest.fixture(scope="module")
def extended(batch, plain):
    """The oracle at 0.3 on the bipartite match of `plain`: (match, n_extra)."""
    return EO.extend(batch["priors"], batch["gt"], batch["n"], np.zeros(batch["B"], np.int32), plain[3], 0.3)


def test_multibox_loss_without_the_key_is_unchanged(gpu, batch, plain):
    torch, _ = gpu
    from multibox_amd import loss as L
    new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, match_iou_threshold=None)
    assert new.n_extra is None
    for x, y in zip(plain, _forward_backward(torch, new, batch)):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal((plain[3] >= 0).sum(1), batch["n"])             # bipartite: one prior per box


def test_multibox_loss_with_the_key(gpu, batch, plain, extended):
    torch, l = gpu
    from multibox_amd import loss as L
    want, want_extra = extended
    assert want_extra.sum() >= 1 and want_extra[1] == 0
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, match_iou_threshold=0.3)
    loss2, dl, dz, match = _forward_backward(torch, ml, batch)
    print("added per image", ml.n_extra.tolist(), "location loss", plain[0][0], "->", loss2[0])
    assert match.tobytes() == want.tobytes() and np.array_equal(ml.n_extra.cpu().numpy(), want_extra)
    # the loss is mbx_loss_fwd_bwd on the extended match: the same entry point, called directly
    B, P, G = batch["B"], batch["P"], batch["G"]
    f = dict(dtype=torch.float32, device="cuda")
    d_loss2, d_dl, d_dz = torch.zeros(2, **f), torch.zeros(B, P, 4, **f), torch.zeros(B, P, **f)
    ws = torch.empty((l.mbx_loss_workspace_bytes(B),), dtype=torch.uint8, device="cuda")
    logits, gt, m = torch.from_numpy(batch["logits"]).cuda(), torch.from_numpy(batch["gt"]).cuda(), torch.from_numpy(want).cuda()
    st = l.mbx_loss_fwd_bwd(ml.decoded.data_ptr(), logits.data_ptr(), 1, gt.data_ptr(), m.data_ptr(), ALPHA, 1.0, B, P, G,
                            d_loss2.data_ptr(), d_dl.data_ptr(), d_dz.data_ptr(), ws.data_ptr(), ws.numel(),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0
    assert loss2.tobytes() == d_loss2.cpu().numpy().tobytes()
    assert dl.tobytes() == d_dl.cpu().numpy().tobytes() and dz.tobytes() == d_dz.cpu().numpy().tobytes()
    assert loss2[0] > plain[0][0]                                         # more positives: a strictly larger location loss


def test_multibox_loss_with_the_key_and_mining(gpu, batch, extended):
    torch, _ = gpu
    from multibox_amd import loss as L
    want, want_extra = extended
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, neg_per_pos=3, match_iou_threshold=0.3)
    _, _, _, match = _forward_backward(torch, ml, batch)
    assert match.tobytes() == want.tobytes()
    n_neg = ml.n_neg.cpu().numpy()
    assert np.array_equal(n_neg, MO.n_selected(want, 3, 0))
    assert np.array_equal(n_neg, 3 * (batch["n"] + want_extra))           # the budget grew with the added positives


def test_extend_matches_wrapper(gpu, batch, plain, extended):
    torch, _ = gpu
    from multibox_amd import loss as L
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    match, n_extra = dev(plain[3]), torch.full((batch["B"],), SENTINEL, dtype=torch.int32, device="cuda")
    out, extra = L.extend_matches(dev(batch["priors"]), dev(batch["gt"]), dev(batch["n"]),
                                  torch.zeros(batch["B"], dtype=torch.int32, device="cuda"), match, 0.3, n_extra)
    torch.cuda.synchronize()
    assert out is match and extra is n_extra
    assert match.cpu().numpy().tobytes() == extended[0].tobytes() and np.array_equal(n_extra.cpu().numpy(), extended[1])
    from multibox_amd import _lib
    with pytest.raises(_lib.MbxError):
        L.extend_matches(dev(batch["priors"]), dev(batch["gt"]), dev(batch["n"]),
                         torch.zeros(batch["B"], dtype=torch.int32, device="cuda"), match, 0.0)


# ---------------------------------------------------------------------------------------------------- through the Trainer
def test_trainer_step_extended_graph_equals_eager(gpu):
    torch, _ = gpu
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
    res = []
    for use_graph in (True, False):
        net = Net(batch=2, input_size=299, k=5, mode="train", seed=5)
        tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, match_iou_threshold=0.3)
        tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0
        match = tr.loss.match.cpu().numpy()
        n_extra = tr.loss.n_extra.cpu().numpy()
        # the bipartite part: mbx_match again on the decoded locations and confidences the step left behind
        bip, st = L.match_boxes(tr.loss.decoded, tr.loss.conf, tr.gt, tr.n_gt, tr.loss.alpha)
        torch.cuda.synchronize()
        bip = bip.cpu().numpy()
        assert int(st.max()) == 0 and (bip >= 0).sum(1).tolist() == [3, 0]
        want, want_extra = EO.extend(priors, gt, n_gt, np.zeros(2, np.int32), bip, 0.3)
        print("added per image", n_extra)
        assert match.tobytes() == want.tobytes() and np.array_equal(n_extra, want_extra)
        assert n_extra[0] > 0 and n_extra[1] == 0
        assert tr.extra_matches_per_image() == float(n_extra.mean())
        res.append((tr.loss.loss2.cpu().numpy(), match, n_extra))
    assert res[0][0].tobytes() == res[1][0].tobytes() and np.isfinite(res[0][0]).all()
    assert res[0][1].tobytes() == res[1][1].tobytes() and np.array_equal(res[0][2], res[1][2])
    # without the key: nothing to report (a second trainer on the last net; it is built, never stepped)
    assert Trainer(net, priors, max_num_bboxes=13, use_graph=False).extra_matches_per_image() is None
