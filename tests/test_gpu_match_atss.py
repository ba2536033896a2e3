"""GPU: mbx_match_atss (ATSS matching behind the bipartite match) against tests/atss_oracle.py.

The C ABI is driven directly with a hand-made `match`, so the first half depends on no matcher.  The bar is exactness: the
kernel's float64 arithmetic has the oracle's operations in the oracle's order, so `match`, `n_extra` and `thr` are compared
byte for byte.  The cases (tests/atss_cases.py): fewer priors than one wavefront on one level (13), a level smaller than
topk with P no multiple of 64 (70), the same on a 1/64 lattice with equal distances on both sides of the cut, the real
priors at 299 px (646, the last level one prior) and at 512 px (3 199, G = 100), topk 1, and topk over every level.
"""
import ctypes as C

import numpy as np
import pytest

from tests import atss_cases as AC
from tests import atss_oracle as AO
from tests import mined_oracle as MO
from tests import loss_cases as LC
from tests.loss_cases import ALPHA, batch, gpu  # noqa: F401  (the fixtures are found by name)

pytestmark = pytest.mark.gpu

SENTINEL = -77
THR_SENTINEL = -7.5


def call(gpu, c, rows=None, with_extra=True, with_thr=True, null=None, levels=None, n_levels=None, topk=None, **override):
    """One call of the C ABI on images `rows` of case c (arrays in `override` replace the case's) ->
    (status, match [B,P], n_extra [B] prefilled with SENTINEL, thr [B,G] prefilled with THR_SENTINEL)."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    get = lambda k: override.get(k, c[k])
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()                 # a copy: the case's arrays are read-only
    priors, gt, n, status, match = dev(get("priors")), dev(get("gt")[rows]), dev(get("n")[rows]), dev(get("status")[rows]), \
        dev(get("match")[rows])
    B, P = match.shape
    n_extra = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    thr = torch.full((B, c["G"]), THR_SENTINEL, dtype=torch.float64, device="cuda")
    levels = c["levels"] if levels is None else levels
    table = (C.c_int32 * len(levels))(*levels)
    ptr = lambda name, t: None if null == name else t.data_ptr()
    st = l.mbx_match_atss(ptr("priors", priors), None if null == "level_start" else table,
                          len(levels) - 1 if n_levels is None else n_levels, ptr("gt", gt), ptr("n_gt", n),
                          ptr("status", status), c["topk"] if topk is None else topk, override.get("B", B),
                          override.get("P", P), override.get("G", c["G"]), ptr("match", match),
                          n_extra.data_ptr() if with_extra else None, thr.data_ptr() if with_thr else None,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, match.cpu().numpy(), n_extra.cpu().numpy(), thr.cpu().numpy()


# --------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", list(AC.CASES))
def test_match_n_extra_and_thr_equal_the_oracle(gpu, name):
    c = AC.make_case(name)
    want, want_extra, want_thr = AC.oracle(name)
    assert want_extra.sum() >= 1 and want_extra[0] == 0                   # the case adds something, or it shows nothing
    st, match, n_extra, thr = call(gpu, c)
    print("added per image", n_extra, "oracle", want_extra)
    assert st == 0
    assert thr.tobytes() == want_thr.tobytes()
    assert match.tobytes() == want.tobytes() and n_extra.tobytes() == want_extra.tobytes()
    had = c["match"] >= 0
    assert np.array_equal(match[had], c["match"][had])                    # what was matched keeps its box


def test_one_candidate_is_a_positive_at_its_own_threshold(gpu):
    c = dict(B=1, P=2, G=1, levels=[0, 2], topk=1, priors=np.array([[0, 0, .5, .5], [.5, .5, 1, 1]], np.float32),
             gt=np.array([[[0, 0, .5, .375]]], np.float32), n=np.array([1], np.int32), status=np.zeros(1, np.int32),
             match=-np.ones((1, 2), np.int32))
    st, match, n_extra, thr = call(gpu, c)
    assert st == 0 and thr.tolist() == [[0.75]] and match.tolist() == [[0, -1]] and n_extra.tolist() == [1]
    on_edge = dict(c, gt=np.array([[[0, 0, .5, .25]]], np.float32))         # y2 == the prior's cy: not inside
    st, match, n_extra, thr = call(gpu, on_edge)
    assert st == 0 and thr.tolist() == [[0.5]] and match.tolist() == [[-1, -1]] and n_extra.tolist() == [0]


# ------------------------------------------------------------------------------------- independence and reproducibility
@pytest.mark.parametrize("name", ["p70", "p646", "p3199"])
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, name):
    c = AC.make_case(name)
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
    c = AC.make_case(name)
    want, want_extra, want_thr = AC.oracle(name)
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
    c = AC.make_case(name)
    B, P = c["B"], c["P"]
    want, want_extra, want_thr = AC.oracle(name)
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
    st, out, n_extra, thr = call(gpu, c, n=n)
    assert st == 0 and out[1].tobytes() == c["match"][1].tobytes() and n_extra[1] == 0 and not thr[1].any()


@pytest.mark.parametrize("name", ["p70", "p646"])
def test_a_nan_in_the_padding_rows_changes_nothing(gpu, name):
    c = AC.make_case(name)
    want, want_extra, want_thr = AC.oracle(name)
    gt = c["gt"].copy()
    for b in range(c["B"]):
        gt[b, c["n"][b]:] = np.nan
    assert np.isnan(gt).any()
    st, match, n_extra, thr = call(gpu, c, gt=gt)
    assert st == 0 and match.tobytes() == want.tobytes() and n_extra.tobytes() == want_extra.tobytes()
    assert thr.tobytes() == want_thr.tobytes()


# --------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("kw", [dict(null="priors"), dict(null="level_start"), dict(null="gt"), dict(null="n_gt"),
                                dict(null="status"), dict(null="match"), dict(B=-1), dict(P=0), dict(G=0), dict(topk=0),
                                dict(n_levels=0), dict(levels=list(range(10)) , P=9), dict(levels=[0, 40, 68, 71]),
                                dict(levels=[1, 40, 68, 70]), dict(levels=[0, 40, 40, 70]), dict(levels=[0, 68, 40, 70])])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, kw):
    c = AC.make_case("p70")
    sentinel = np.full((4, 70), SENTINEL, np.int32)
    st, match, n_extra, thr = call(gpu, c, match=sentinel, **kw)
    assert st == -1
    assert np.all(match == SENTINEL) and np.all(n_extra == SENTINEL) and np.all(thr == THR_SENTINEL)


def test_an_unsupported_size_is_refused_and_nothing_is_written(gpu):
    torch, l = gpu
    c = AC.make_case("p70")
    sentinel = np.full((4, 70), SENTINEL, np.int32)
    # G is refused before any pointer is followed: nothing is launched, so the small buffers are never indexed
    st, match, n_extra, thr = call(gpu, c, match=sentinel, G=1 << 20)
    assert st == -2 and l.mbx_match_atss_supported(70, 1 << 20, 3, (C.c_int32 * 4)(*c["levels"]), 4) == -2
    assert np.all(match == SENTINEL) and np.all(n_extra == SENTINEL) and np.all(thr == THR_SENTINEL)
    st, match, n_extra, thr = call(gpu, c)                                 # the same call with the real G writes
    assert st == 0 and not np.any(n_extra == SENTINEL)
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    f = torch.zeros(8, dtype=torch.float32, device="cuda")
    assert l.mbx_match_atss(f.data_ptr(), (C.c_int32 * 2)(0, 1), 1, f.data_ptr(), z.data_ptr(), z.data_ptr(), 9, 0, 1, 1,
                            z.data_ptr(), None, None, None) == 0           # B == 0


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
def selected(batch, plain):
    """The oracle at topk 9 on the bipartite match of `plain`: (match, n_extra, thr)."""
    return AO.atss(batch["priors"], AC.LEVELS_299, batch["gt"], batch["n"], np.zeros(batch["B"], np.int32), plain[3], 9)


def test_multibox_loss_without_the_key_is_unchanged(gpu, batch, plain):
    torch, _ = gpu
    from multibox_amd import loss as L
    new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, atss_topk=None, prior_levels=None)
    assert new.n_atss is None and new.atss_thr is None
    for x, y in zip(plain, _forward_backward(torch, new, batch)):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal((plain[3] >= 0).sum(1), batch["n"])             # bipartite: one prior per box


def test_multibox_loss_with_the_key(gpu, batch, plain, selected):
    torch, l = gpu
    from multibox_amd import loss as L
    want, want_extra, want_thr = selected
    assert want_extra.sum() >= 1 and want_extra[1] == 0
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, atss_topk=9, prior_levels=AC.LEVELS_299)
    loss2, dl, dz, match = _forward_backward(torch, ml, batch)
    print("added per image", ml.n_atss.tolist(), "location loss", plain[0][0], "->", loss2[0])
    assert match.tobytes() == want.tobytes() and np.array_equal(ml.n_atss.cpu().numpy(), want_extra)
    assert ml.atss_thr.cpu().numpy().tobytes() == want_thr.tobytes()
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


def test_multibox_loss_with_the_key_and_mining(gpu, batch, selected):
    torch, _ = gpu
    from multibox_amd import loss as L
    want, want_extra, _ = selected
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, neg_per_pos=3, atss_topk=9, prior_levels=AC.LEVELS_299)
    _, _, _, match = _forward_backward(torch, ml, batch)
    assert match.tobytes() == want.tobytes()
    n_neg = ml.n_neg.cpu().numpy()
    assert np.array_equal(n_neg, MO.n_selected(want, 3, 0))
    assert np.array_equal(n_neg, 3 * (batch["n"] + want_extra))           # the budget grew with the added positives
    assert np.array_equal(n_neg, 3 * (batch["n"] + ml.n_atss.cpu().numpy()))


def test_multibox_loss_with_the_key_focal_and_giou(gpu, batch, selected):
    torch, l = gpu
    from multibox_amd import loss as L
    want, _, _ = selected
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, atss_topk=9, prior_levels=AC.LEVELS_299,
                        focal_gamma=2.0, focal_alpha=0.25, loc_loss="giou")
    loss2, dl, dz, match = _forward_backward(torch, ml, batch)
    assert match.tobytes() == want.tobytes()
    B, P, G = batch["B"], batch["P"], batch["G"]
    f = dict(dtype=torch.float32, device="cuda")
    d_loss2, d_dl, d_dz = torch.zeros(2, **f), torch.zeros(B, P, 4, **f), torch.zeros(B, P, **f)
    ws = torch.empty((l.mbx_loss_loc_workspace_bytes(B, P),), dtype=torch.uint8, device="cuda")
    logits, gt, m = torch.from_numpy(batch["logits"]).cuda(), torch.from_numpy(batch["gt"]).cuda(), torch.from_numpy(want).cuda()
    st = l.mbx_loss_fwd_bwd_loc(ml.decoded.data_ptr(), logits.data_ptr(), 1, gt.data_ptr(), m.data_ptr(), ALPHA, 1.0, B, P, G,
                                d_loss2.data_ptr(), d_dl.data_ptr(), d_dz.data_ptr(), L.LOC_TYPES.index("giou"), 0.0, 2.0, 0.25,
                                0.75, 0, 0, None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0 and np.isfinite(loss2).all()
    assert loss2.tobytes() == d_loss2.cpu().numpy().tobytes()
    assert dl.tobytes() == d_dl.cpu().numpy().tobytes() and dz.tobytes() == d_dz.cpu().numpy().tobytes()


def test_atss_matches_wrapper(gpu, batch, plain, selected):
    torch, _ = gpu
    from multibox_amd import loss as L, _lib
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, G = batch["B"], batch["G"]
    match, n_extra = dev(plain[3]), torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    thr = torch.full((B, G), THR_SENTINEL, dtype=torch.float64, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    out, extra, t = L.atss_matches(dev(batch["priors"]), AC.LEVELS_299, dev(batch["gt"]), dev(batch["n"]), status, match, 9,
                                   n_extra, thr)
    torch.cuda.synchronize()
    assert out is match and extra is n_extra and t is thr
    assert match.cpu().numpy().tobytes() == selected[0].tobytes() and np.array_equal(n_extra.cpu().numpy(), selected[1])
    assert thr.cpu().numpy().tobytes() == selected[2].tobytes()
    with pytest.raises(_lib.MbxError):
        L.atss_matches(dev(batch["priors"]), AC.LEVELS_299, dev(batch["gt"]), dev(batch["n"]), status, match, 0)


# ---------------------------------------------------------------------------------------------------- through the Trainer
def test_trainer_step_with_atss_graph_equals_eager(gpu):
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
        tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, atss_topk=9)
        assert tr.loss.prior_levels == AC.LEVELS_299                      # derived from the network's heads
        tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0
        match = tr.loss.match.cpu().numpy()
        n_atss = tr.loss.n_atss.cpu().numpy()
        # the bipartite part: mbx_match again on the decoded locations and confidences the step left behind
        bip, st = L.match_boxes(tr.loss.decoded, tr.loss.conf, tr.gt, tr.n_gt, tr.loss.alpha)
        torch.cuda.synchronize()
        bip = bip.cpu().numpy()
        assert int(st.max()) == 0 and (bip >= 0).sum(1).tolist() == [3, 0]
        want, want_extra, want_thr = AO.atss(priors, AC.LEVELS_299, gt, n_gt, np.zeros(2, np.int32), bip, 9)
        print("added per image", n_atss)
        assert match.tobytes() == want.tobytes() and np.array_equal(n_atss, want_extra)
        assert tr.loss.atss_thr.cpu().numpy().tobytes() == want_thr.tobytes()
        assert n_atss[0] > 0 and n_atss[1] == 0
        assert tr.atss_matches_per_image() == float(n_atss.mean()) and tr.extra_matches_per_image() is None
        res.append((tr.loss.loss2.cpu().numpy(), match, n_atss))
    assert res[0][0].tobytes() == res[1][0].tobytes() and np.isfinite(res[0][0]).all()
    assert res[0][1].tobytes() == res[1][1].tobytes() and np.array_equal(res[0][2], res[1][2])
    # without the key: nothing to report (a second trainer on the last net; it is built, never stepped)
    assert Trainer(net, priors, max_num_bboxes=13, use_graph=False).atss_matches_per_image() is None
