"""mbx_match, mbx_decode_filter_topk, mbx_nms and mbx_decode_conf at the boundaries of their launch shapes, on ties and on
special values.  Every device result is compared with tests/postproc_oracle.py (numpy / float64, oracle.ref_numpy, scipy),
never with another device result, except where a test is about determinism or about the place of an image in the batch.
The inputs come from the builders of that file; tests/test_postproc_oracle_cpu.py proves their preconditions on the CPU."""
import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import postproc_oracle as O

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from multibox_amd import _lib

    class Gpu:
        pass
    Gpu.torch, Gpu.lib = torch, _lib.lib()
    Gpu.dev = staticmethod(lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    Gpu.stream = staticmethod(lambda: torch.cuda.current_stream().cuda_stream)
    return Gpu


def ptr(t):
    return None if t is None else t.data_ptr()


# =========================================================================================================== mbx_match
def run_match(gpu, dec, conf, gt, n, alpha):
    """One launch into sentinel-filled outputs: (rc, match [B,P], status [B])."""
    B, P, G = dec.shape[0], dec.shape[1], gt.shape[1]
    m = gpu.torch.full((B, P), -7, dtype=gpu.torch.int32, device="cuda")
    st = gpu.torch.full((B,), -7, dtype=gpu.torch.int32, device="cuda")
    d = [gpu.dev(np.asarray(a, dt)) for a, dt in ((dec, np.float32), (conf, np.float32), (gt, np.float32), (n, np.int32))]
    rc = gpu.lib.mbx_match(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), float(alpha), B, P, G,
                           m.data_ptr(), st.data_ptr(), None, 0, gpu.stream())
    gpu.torch.cuda.synchronize()
    return rc, m.cpu().numpy(), st.cpu().numpy()


def oracle_match(dec, conf, gt, n, alpha):
    with np.errstate(over="ignore", invalid="ignore"):
        return R.compute_assignments(dec.reshape(-1, 4), conf.reshape(-1), gt, n, dec.shape[0], alpha)[2]


@pytest.mark.parametrize("B,P,G", O.MATCH_SHAPES)
def test_match_launch_shapes(gpu, B, P, G):
    """a.  Tie-free inputs at every size where the host or the kernel takes another path (postproc_oracle.MATCH_SHAPES says
    where each comes from): exact equality with scipy, through multibox_amd.loss.match_boxes."""
    from multibox_amd import loss as L
    dec, conf, gt, n = O.match_launch_case(B, P, G)
    m, st = L.match_boxes(gpu.dev(dec), gpu.dev(conf), gpu.dev(gt), gpu.dev(n), 1000.0)
    assert st.cpu().tolist() == [0] * B
    assert np.array_equal(m.cpu().numpy(), oracle_match(dec, conf, gt, n, 1000.0))
    rc, m2, st2 = run_match(gpu, dec, conf, gt, n, 1000.0)               # the same through the C ABI, into sentinels
    assert rc == OK and np.array_equal(m2, m.cpu().numpy()) and not st2.any()


def test_match_above_the_largest_size_is_refused(gpu):
    B, P, G = O.MATCH_TOO_BIG
    assert O.match_lds_bytes(P, G) > 150 * 1024 >= O.match_lds_bytes(P - 1, G)
    rc, m, st = run_match(gpu, np.zeros((B, P, 4), np.float32), np.full((B, P), 0.5, np.float32), np.zeros((B, G, 4), np.float32),
                          np.array([3], np.int32), 1000.0)
    assert rc == UNSUPPORTED and (m == -7).all() and (st == -7).all()


@pytest.mark.parametrize("alpha", [1000.0, 1e-3])
def test_match_contention(gpu, alpha):
    """b.  100 gt boxes inside a 0.01 neighbourhood of one box, 646 predictions: every gt wants the same predictions, the
    augmenting paths are long.  Tie-free in the sense of postproc_oracle.match_contention_case: exact equality."""
    dec, conf, gt, n, _ = O.match_contention_case(alpha)
    rc, m, st = run_match(gpu, dec, conf, gt, n, alpha)
    assert rc == OK and st.tolist() == [0]
    assert np.array_equal(m, oracle_match(dec, conf, gt, n, alpha))


TIE_CASES = ["twin_gt", "twin_predictions", "all_equal", "start_of_training", "contention_flat"]


@pytest.mark.parametrize("name", TIE_CASES)
def test_match_ties(gpu, golden, name):
    """c.  Equal costs: the kernel's choice among the optimal assignments is its own (cand_better: a free column first, then
    the lowest index) and need not be scipy's, so what is asserted is that it IS optimal: valid, and on the oracle's cost
    matrix within 8 n ulp32(max|C|) of scipy's total (postproc_oracle.tie_bound says where the bound comes from); then that
    the choice is the same on every call and wherever the image stands in a batch.
    Measured on the MI355X: the difference of the totals is exactly 0 in all five cases (bounds 1.9e-5 to 2.9e-3); scipy's
    own choice is reproduced in four of them and not in `contention_flat` (100 boxes, rows of equal float32 costs), which
    is why equality with scipy is NOT asserted and include/mbx.h says that the choice among equals is the kernel's own."""
    dec, conf, gt, alpha = O.match_tie_cases(golden.priors["k5_restrict"])[name]
    P, n = len(dec), len(gt)
    C = O.costs(dec, conf, gt, n, alpha)
    rc, m, st = run_match(gpu, dec[None], conf[None], gt[None], [n], alpha)
    assert rc == OK and st.tolist() == [0]
    total = O.assignment_cost(C, m[0])                                    # 1. valid
    want, bound = O.scipy_total(C), O.tie_bound(C, n)
    same = np.array_equal(m, oracle_match(dec[None], conf[None], gt[None], [n], alpha))
    print("\ntie case %s: device total - scipy total = %.3g (bound %.3g); scipy's own choice reproduced: %s"
          % (name, total - want, bound, same))
    assert abs(total - want) <= bound, "device %.17g scipy %.17g difference %.3g bound %.3g" % (total, want, total - want, bound)
    rc, m2, st2 = run_match(gpu, dec[None], conf[None], gt[None], [n], alpha)
    assert rc == OK and m2.tobytes() == m.tobytes() and st2.tolist() == [0]                  # 3. the same bytes on every call
    fd, fc, fg = O.random_image(P, n, O.MATCH_SEED + 5)                   # 4. third of four images, beside others
    bd, bc, bg = np.stack([fd, fd[::-1], dec, fd]), np.stack([fc, fc[::-1], conf, fc]), np.stack([fg, fg, gt, fg[::-1]])
    rc, m4, st4 = run_match(gpu, bd, bc, bg, [n, max(n - 1, 0), n, n], alpha)
    assert rc == OK and not st4.any() and m4[2].tobytes() == m[0].tobytes()


def test_match_status_and_padding(gpu):
    """d.  One launch of nine images, P = 40, G = 8."""
    P, G, n = 40, 8, 5
    pad = lambda g: np.concatenate([g, np.zeros((G - len(g), 4), np.float32)])
    plain, one, far1, far = [O.match_special_case(k) for k in ("plain", "conf_one", "far_one", "far_all")]
    junk = pad(plain[2])
    junk[n:] = [[np.nan, 0, 1, 2], [np.inf, -np.inf, 0, 0], [np.nan] * 4]
    zero_conf = plain[1].copy()
    zero_conf[9] = 0.0
    images = [(plain[0], plain[1], pad(plain[2]), n),       # 0: the plain image
              (plain[0], plain[1], pad(plain[2]), -3),      # 1: n < 0 -> status 0, nothing matched
              (plain[0], plain[1], pad(plain[2]), G + 1),   # 2: G < n <= P -> status 1
              (plain[0], plain[1], junk, n),                # 3: NaN and inf in the padding rows of gt: never read
              (plain[0], zero_conf, pad(plain[2]), n),      # 4: a confidence of exactly 0: log 0 -> status 2
              (one[0], one[1], pad(one[2]), n),             # 5: confidences of exactly 1 and of 1.5
              (far1[0], far1[1], pad(far1[2]), n),          # 6: one prediction whose costs are +inf
              (far[0], far[1], pad(far[2]), n),             # 7: every prediction there: infeasible
              (plain[0], plain[1], pad(plain[2]), P + 1)]   # 8: n > P -> status 1
    dec, conf, gt = [np.stack([im[k] for im in images]) for k in range(3)]
    nn = np.array([im[3] for im in images], np.int32)
    rc, m, st = run_match(gpu, dec, conf, gt, nn, 1000.0)
    assert rc == OK and st.tolist() == [0, 0, 1, 0, 2, 0, 0, 2, 1]
    for b in np.nonzero(st)[0]:
        assert (m[b] == -1).all(), b
    assert (m[1] == -1).all()
    assert m[3].tobytes() == m[0].tobytes()
    for b in (0, 5, 6):
        want = oracle_match(dec[b:b + 1], conf[b:b + 1], gt[b:b + 1], nn[b:b + 1], 1000.0)
        assert np.array_equal(m[b:b + 1], want), b
    assert m[5, 3] >= 0 and m[5, 17] >= 0 and m[6, 11] == -1


# ========================================================================================== mbx_decode_filter_topk
def run_topk(gpu, raw, conf, priors, meta, k_max):
    """One launch into sentinel-filled outputs: (rc, boxes [B,k_max,4] f64, scores, index, count)."""
    from multibox_amd import detect as D
    B, P = raw.shape[:2]
    t = gpu.torch
    ob = t.full((B, k_max, 4), 7.0, dtype=t.float64, device="cuda")
    os_ = t.full((B, k_max), 7.0, dtype=t.float32, device="cuda")
    oi = t.full((B, k_max), 7, dtype=t.int32, device="cuda")
    oc = t.full((B,), 7, dtype=t.int32, device="cuda")
    d_meta = D.make_patch_meta(meta["offsets"], meta["dims"], meta["flips"], meta["res"], meta["mtk"], meta["hw"])
    d = [gpu.dev(np.asarray(a, np.float32)) for a in (raw, conf, priors)]
    rc = gpu.lib.mbx_decode_filter_topk(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_meta.data_ptr(), B, P, k_max,
                                        ob.data_ptr(), os_.data_ptr(), oi.data_ptr(), oc.data_ptr(), gpu.stream())
    t.cuda.synchronize()
    return (rc,) + tuple(x.cpu().numpy() for x in (ob, os_, oi, oc))


def check_topk(gpu, raw, conf, priors, meta, k_max):
    """Every slot of the four outputs against the oracle: index[:count] exact, scores and boxes as bytes, count, and all
    slots at or past count 0.0 / 0.0f / -1 (the expected arrays hold exactly that)."""
    eb, es, ei, ec = O.topk_expected(raw, conf, priors, meta, k_max)
    rc, ob, os_, oi, oc = run_topk(gpu, raw, conf, priors, meta, k_max)
    assert rc == OK
    assert np.array_equal(oc, ec), (oc.tolist(), ec.tolist())
    assert np.array_equal(oi, ei)
    assert os_.tobytes() == es.tobytes()
    assert ob.tobytes() == eb.tobytes()
    return ob, os_, oi, oc


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1024, 8192, 8193, 16384])
def test_topk_sizes(gpu, P):
    """P below the workgroup (64 sort keys, 32 working threads), at and next to powers of two, and in (8192, 16384], where
    the 128 KiB of sort keys need more LDS than a launch gets without asking."""
    raw, conf, priors, meta = O.topk_random_case(3, P, seed=P)
    oc = check_topk(gpu, raw, conf, priors, meta, 200)[3]
    assert P < 300 or oc.min() == 200


def test_topk_above_the_largest_size_is_refused(gpu):
    raw, conf, priors, meta = O.topk_random_case(1, 16385, seed=1)
    rc, ob, os_, oi, oc = run_topk(gpu, raw, conf, priors, meta, 8)
    assert rc == UNSUPPORTED and (ob == 7.0).all() and (os_ == 7.0).all() and (oi == 7).all() and (oc == 7).all()


@pytest.mark.parametrize("k_max", [1, 7, 200, 300])
@pytest.mark.parametrize("P", [257, 65])
def test_topk_kmax_and_max_to_keep(gpu, P, k_max):
    """count = clamp(min(kept, max_to_keep), 0, k_max), with k_max below, at and above max_to_keep and above P."""
    raw, conf, priors, meta = O.topk_random_case(6, P, seed=100 + P)
    meta["mtk"][:] = [-3, 0, 1, k_max - 1, k_max, k_max + 50]
    oc = check_topk(gpu, raw, conf, priors, meta, k_max)[3]
    assert oc[0] == 0 and oc[1] == 0 and oc[2] == 1 and (oc <= min(k_max, P)).all()


def test_topk_filter_is_strict(gpu):
    raw, conf, priors, meta, _ = O.topk_boundary_case()
    ob, os_, oi, oc = check_topk(gpu, raw, conf, priors, meta, 16)
    assert oc.tolist() == [9, 4, 9]                                       # on the restriction: kept; one ulp outside: dropped
    assert sorted(oi[1, :4].tolist()) == [5, 6, 7, 8]


def test_topk_clips_before_it_filters(gpu):
    priors = np.tile(np.array([[0.2, 0.2, 0.8, 0.8]], np.float32), (70, 1))
    raw = np.zeros((2, 70, 4), np.float32)
    raw[0, :, :2], raw[0, :, 2:] = -0.5, 0.9                              # decoded -0.3 and 1.7
    raw[1] = raw[0] * np.float32(0.5)                                     # decoded -0.05 and 1.25
    conf = R.sigmoid_f32(np.random.RandomState(3).randn(2, 70))
    ob, os_, oi, oc = check_topk(gpu, raw, conf, priors, O.make_meta(2, dims=(100, 100)), 128)
    assert oc.tolist() == [70, 70] and (ob[:, :70] == np.array([0.0, 0.0, 1.0, 1.0])).all()


def test_topk_geometry_offset_flip_and_odd_ratios(gpu):
    """A 250 x 280 patch at offset (37, 113) of a 412 x 500 image, plain and flipped in one launch: no ratio is dyadic."""
    raw, conf, priors, _ = O.topk_random_case(2, 333, seed=9)
    meta = O.make_meta(2, offsets=(37, 113), dims=(250, 280), flips=[0, 1], hw=(412, 500), mtk=150)
    raw[1], conf[1] = raw[0], conf[0]
    ob, os_, oi, oc = check_topk(gpu, raw, conf, priors, meta, 200)
    assert oc.tolist() == [150, 150] and np.array_equal(oi[0], oi[1])
    idx = oi[0, :150]
    for b in (0, 1):
        want = R.convert_proposals(R.decode_clip(raw[b], priors)[idx], (37, 113), (250, 280), (412, 500), b)
        assert ob[b, :150].tobytes() == want.tobytes()
    assert np.array_equal(ob[1, :150, 0], 1.0 - ob[0, :150, 2]) and np.array_equal(ob[1, :150, 1], ob[0, :150, 1])


def test_topk_ties_across_the_cut(gpu):
    """Among equal scores the higher prediction index comes first, also where max_to_keep cuts through the tie group; +0.0
    and -0.0 are one score."""
    raw, conf, priors, meta = O.topk_random_case(3, 400, seed=11)
    meta["res"][:] = [0, 0, 1, 1]
    conf[0, 50:350] = 0.5                                                 # 300 equal scores, cut at 200 inside the group
    conf[0, :50], conf[0, 350:] = 0.75, 0.25
    conf[1, :] = 0.5
    conf[2, :] = np.where(np.arange(400) % 3 == 0, np.float32(-0.0), np.float32(0.0))
    ob, os_, oi, oc = check_topk(gpu, raw, conf, priors, meta, 200)
    assert oc.tolist() == [200, 200, 200]
    assert oi[0].tolist() == list(range(49, -1, -1)) + list(range(349, 199, -1))
    assert oi[1].tolist() == oi[2].tolist() == list(range(399, 199, -1))
    assert os_[2].tobytes() == conf[2, oi[2]].tobytes() and np.signbit(os_[2]).any() and not np.signbit(os_[2]).all()


def test_topk_everything_dropped(gpu):
    raw, conf, priors, meta = O.topk_random_case(3, 130, seed=12)
    meta["res"][1] = [0.99, 0.99, 1.0, 1.0]                               # no box starts that far right
    ob, os_, oi, oc = check_topk(gpu, raw, conf, priors, meta, 64)
    assert oc[1] == 0 and not ob[1].any() and not os_[1].any() and (oi[1] == -1).all() and oc[0] == 64


def test_topk_place_in_the_batch_and_determinism(gpu):
    raw, conf, priors, meta = O.topk_random_case(3, 257, seed=13)
    first = check_topk(gpu, raw, conf, priors, meta, 200)
    again = run_topk(gpu, raw, conf, priors, meta, 200)[1:]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    order = np.array([2, 0, 1, 1, 0])
    moved = check_topk(gpu, raw[order], conf[order], priors, O.take_meta(meta, order), 200)
    for a, b in zip(first, moved):
        assert a[order].tobytes() == b.tobytes()


def test_topk_nan_coordinate_is_clipped_to_zero(gpu):
    """The kernel clips with fminf(fmaxf(x, 0), 1), which turns a NaN coordinate into 0 (numpy's clip keeps the NaN, and a
    NaN passes the reference's strict filter whatever the restriction).  Pinned: the outputs are the oracle's for the input
    with every NaN coordinate replaced by one that clips to 0."""
    raw, conf, priors, meta = O.topk_random_case(2, 70, seed=14)           # patch 0: (0, 0, 1, 1); patch 1: (.1, .1, .9, .9)
    for b in (0, 1):
        raw[b, [5, 9, 20]] = np.array([0.3, 0.3, 0.6, 0.6], np.float32) - priors[[5, 9, 20]]      # well inside both restrictions
        raw[b, 5, 0] = raw[b, 9, 2] = raw[b, 20, :] = np.nan
    conf[:, [5, 9, 20]] = 0.99999                                         # where kept, they come first
    as_zero = np.where(np.isnan(raw), np.float32(-1.0), raw)
    eb, es, ei, ec = O.topk_expected(as_zero, conf, priors, meta, 64)
    rc, ob, os_, oi, oc = run_topk(gpu, raw, conf, priors, meta, 64)
    assert rc == OK and np.array_equal(oc, ec) and np.array_equal(oi, ei)
    assert os_.tobytes() == es.tobytes() and ob.tobytes() == eb.tobytes() and not np.isnan(ob).any()
    assert {5, 20} <= set(oi[0, :3].tolist()) and ob[0, oi[0].tolist().index(20)].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert not {5, 20} & set(oi[1].tolist()) and oi[1, 0] == 9            # x1 = 0 is outside (.1, .1, .9, .9): dropped; x2 = 0 is not
    with np.errstate(invalid="ignore"):
        ref_idx = O.topk_expected(raw, conf, priors, meta, 64)[2]
    assert {5, 9, 20} <= set(ref_idx[1].tolist())                         # the numpy reference keeps them: the difference


# ============================================================================================================ mbx_nms
def run_nms(gpu, boxes, scores, index, count, k_max, thr):
    d = [gpu.dev(np.asarray(a, dt).copy()) for a, dt in ((boxes, np.float64), (scores, np.float32), (index, np.int32), (count, np.int32))]
    rc = gpu.lib.mbx_nms(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(count), k_max, float(thr), gpu.stream())
    gpu.torch.cuda.synchronize()
    return (rc,) + tuple(x.cpu().numpy() for x in d)


def nms_rows(pattern, k_max, counts):
    """len(counts) rows of the same k_max boxes, scores descending, index = slot."""
    B = len(counts)
    boxes = np.tile(O.nms_boxes(pattern, k_max)[None], (B, 1, 1))
    scores = np.tile(np.linspace(0.99, 0.01, k_max, dtype=np.float32)[None], (B, 1))
    index = np.tile(np.arange(k_max, dtype=np.int32)[None], (B, 1)) + 1000 * np.arange(B, dtype=np.int32)[:, None]
    return boxes, scores, index, np.array(counts, np.int32)


def check_nms(gpu, boxes, scores, index, count, k_max, thr, greedy=O.nms_greedy_vec):
    rc, ob, os_, oi, oc = run_nms(gpu, boxes, scores, index, count, k_max, thr)
    assert rc == OK
    for b, (c, eb, es, ei) in enumerate(O.nms_expected(boxes, scores, index, count, k_max, thr, greedy)):
        assert oc[b] == c, (thr, b, int(oc[b]), c)
        assert np.array_equal(oi[b, :c], ei), (thr, b)
        assert ob[b, :c].tobytes() == eb.tobytes() and os_[b, :c].tobytes() == es.tobytes(), (thr, b)
    return ob, os_, oi, oc


NMS_KMAX = [1, 64, 65, 256, 257, 512] + list(O.nms_lds_crossing()) + [1024]


@pytest.mark.parametrize("k_max", NMS_KMAX)
def test_nms_sizes_counts_and_patterns(gpu, k_max):
    """k_max from one box to the largest: one word per bit row and up to 16 (the one-wave walk reads words owned by other
    lanes from 5 up), one compaction sweep and up to four, and both sides of the LDS size a launch gets without asking --
    postproc_oracle.nms_lds_crossing() re-derives that pair, (704, 705), from the host's (k_max * W + W) * 8 with
    W = ceil(k_max / 64).  Rows with counts 0, 1, k_max, and k_max + 5, -2 and -100 (clamped)."""
    counts = [0, 1, k_max, k_max + 5, -2, -100]
    for pattern in O.NMS_PATTERNS:
        rows = nms_rows(pattern, k_max, counts)
        for thr in O.NMS_THRESHOLDS:
            ob, os_, oi, oc = check_nms(gpu, *rows, k_max, thr)
            assert oc[0] == 0 and oc[1] == 1 and oc[4] == 0 and oc[5] == 0 and oc[2] == oc[3]
            if k_max <= 65:                                               # and against ref_numpy.nms_greedy itself
                check_nms(gpu, *rows, k_max, thr, R.nms_greedy)
            if pattern == "chain" and thr == 0.5:
                assert oi[2, :oc[2]].tolist() == list(range(2000, 2000 + k_max, 2))          # every other box
            if pattern == "identical":
                assert oc[2] == (k_max if thr == 1.0 else 1)
            if pattern == "disjoint":
                assert oc[2] == k_max


def test_nms_above_the_largest_size_is_refused(gpu):
    rows = nms_rows("chain", 1025, [1025, 3])
    rc, ob, os_, oi, oc = run_nms(gpu, *rows, 1025, 0.5)
    assert rc == UNSUPPORTED
    assert all(a.tobytes() == b.tobytes() for a, b in zip((ob, os_, oi, oc), rows))


def test_nms_iou_exactly_at_the_threshold(gpu):
    boxes = np.array([[[0, 0, 1, 1], [0, 0, 1, 0.5]]] * 2, np.float64)
    scores, index, count = np.array([[0.9, 0.8]] * 2, np.float32), np.array([[0, 1]] * 2, np.int32), np.array([2, 2], np.int32)
    assert check_nms(gpu, boxes, scores, index, count, 2, 0.5, R.nms_greedy)[3].tolist() == [2, 2]         # 0.5 > 0.5 is false
    assert check_nms(gpu, boxes, scores, index, count, 2, float(np.nextafter(0.5, 0.0)), R.nms_greedy)[3].tolist() == [1, 1]


def test_nms_place_in_the_batch_and_determinism(gpu):
    k_max = 300
    boxes = np.stack([O.nms_boxes(p, k_max) for p in ("clustered", "chain", "last_sweep", "identical")])
    scores = np.tile(np.linspace(0.99, 0.01, k_max, dtype=np.float32)[None], (4, 1))
    index = np.tile(np.arange(k_max, dtype=np.int32)[None], (4, 1))
    count = np.array([300, 257, 300, 64], np.int32)
    first = check_nms(gpu, boxes, scores, index, count, k_max, 0.5)
    again = run_nms(gpu, boxes, scores, index, count, k_max, 0.5)[1:]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    order = np.array([3, 1, 0, 2, 1])
    moved = check_nms(gpu, boxes[order], scores[order], index[order], count[order], k_max, 0.5)
    for a, b in zip(first, moved):
        assert a[order].tobytes() == b.tobytes()


# ==================================================================================================== mbx_decode_conf
def run_decode_conf(gpu, raw, logits, priors, B, P, eps, want_decoded=True, want_conf=True):
    """(rc, decoded [B,P,4], conf [B,P]) from sentinel-filled outputs; an output that is not wanted is passed as NULL and
    returned as it was."""
    t = gpu.torch
    n = max(B, 1) * max(P, 1)
    dec = t.full((n, 4), 7.0, dtype=t.float32, device="cuda")
    cf = t.full((n,), 7.0, dtype=t.float32, device="cuda")
    d = [None if a is None else gpu.dev(np.asarray(a, np.float32)) for a in (raw, logits, priors)]
    rc = gpu.lib.mbx_decode_conf(ptr(d[0]), ptr(d[1]), ptr(d[2]), B, P, float(eps), dec.data_ptr() if want_decoded else None,
                                 cf.data_ptr() if want_conf else None, gpu.stream())
    t.cuda.synchronize()
    return rc, dec.cpu().numpy(), cf.cpu().numpy()


@pytest.fixture(scope="module")
def big_decode_inputs():
    B, P = 130, 4096                                                      # 532 480 elements > 2048 workgroups x 256 threads
    assert B * P > 2048 * 256
    rng = np.random.RandomState(21)
    raw = (rng.randn(B, P, 4) * 0.1).astype(np.float32)
    priors = rng.uniform(0, 1, (P, 4)).astype(np.float32)
    logits = (rng.randn(B, P) * 6).astype(np.float32)
    logits.reshape(-1)[::1001] = rng.uniform(-104, 90, len(logits.reshape(-1)[::1001]))       # the tails: denormal results
    return raw, logits, priors


@pytest.mark.parametrize("eps", [1e-10, 0.0])
def test_decode_conf_grid_stride_loop(gpu, big_decode_inputs, eps):
    """The grid is capped at 2048 workgroups, so the last 8 192 elements are reached by the second trip of the loop only.
    decoded is the float32 sum, bit for bit; conf within 4 ulp32(ref) + 2^-126 of sigmoid_ref: 1 ulp for expf as documented,
    one rounding each for the add, the divide and the epsilon add, and the smallest normal for flushed denormals.
    Measured on the MI355X: the largest error is 3 ulp32 with eps_add = 1e-10 and 2 ulp32 with 0."""
    raw, logits, priors = big_decode_inputs
    B, P = logits.shape
    rc, dec, cf = run_decode_conf(gpu, raw, logits, priors, B, P, eps)
    assert rc == OK
    assert dec.reshape(B, P, 4).tobytes() == (raw + priors[None]).astype(np.float32).tobytes()
    ref = O.sigmoid_ref(logits, eps).reshape(-1)
    ulp = np.spacing(np.abs(ref)).astype(np.float64)
    err = np.abs(cf.astype(np.float64) - ref.astype(np.float64))
    print("\nmbx_decode_conf eps_add %g: largest error %.3f ulp32 (beyond the 2^-126 allowance)"
          % (eps, float((np.maximum(err - 2.0 ** -126, 0) / ulp).max())))
    assert (err <= 4 * ulp + 2.0 ** -126).all(), float((err / ulp).max())
    assert (cf[-8192:] != 7.0).all()


def test_decode_conf_special_values(gpu):
    z = np.array([[0.0, np.inf, -np.inf, -200.0, np.nan]], np.float32)
    for eps in (np.float32(1e-10), np.float32(0.0)):
        rc, _, cf = run_decode_conf(gpu, None, z, None, 1, 5, eps, want_decoded=False)
        assert rc == OK
        assert cf[0] == np.float32(0.5) + eps and cf[1] == np.float32(1.0) + eps and cf[2] == eps and cf[3] == eps
        assert np.isnan(cf[4])
        assert cf[:4].tobytes() == O.sigmoid_ref(z, eps)[0, :4].tobytes()


def test_decode_conf_null_outputs_and_argument_checks(gpu):
    rng = np.random.RandomState(22)
    B, P = 3, 70
    raw, priors = rng.randn(B, P, 4).astype(np.float32), rng.rand(P, 4).astype(np.float32)
    z = rng.randn(B, P).astype(np.float32)
    rc, dec, cf = run_decode_conf(gpu, raw, None, priors, B, P, 1e-10, want_conf=False)      # only decoded; no logits needed
    assert rc == OK and dec.reshape(B, P, 4).tobytes() == (raw + priors[None]).astype(np.float32).tobytes() and (cf == 7.0).all()
    rc, dec, cf = run_decode_conf(gpu, None, z, None, B, P, 1e-10, want_decoded=False)       # only conf; no raw or priors needed
    assert rc == OK and (dec == 7.0).all() and (cf != 7.0).all()
    err = np.abs(cf.astype(np.float64) - O.sigmoid_ref(z, 1e-10).reshape(-1))
    assert (err <= 4 * np.spacing(np.abs(O.sigmoid_ref(z, 1e-10).reshape(-1)))).all()
    rc, dec, cf = run_decode_conf(gpu, raw, z, priors, B, P, 1e-10, want_decoded=False, want_conf=False)
    assert rc == OK and (dec == 7.0).all() and (cf == 7.0).all()                             # neither: nothing launched
    for args in ((None, z, priors), (raw, z, None)):                                          # decoded without raw / priors
        rc, dec, cf = run_decode_conf(gpu, *args, B, P, 1e-10)
        assert rc == INVALID and (dec == 7.0).all() and (cf == 7.0).all()
    rc, dec, cf = run_decode_conf(gpu, raw, None, priors, B, P, 1e-10)                       # conf without logits
    assert rc == INVALID and (dec == 7.0).all() and (cf == 7.0).all()
    for b, p, want in ((-1, P, INVALID), (B, 0, INVALID), (B, -5, INVALID), (0, P, OK)):
        rc, dec, cf = run_decode_conf(gpu, raw, z, priors, b, p, 1e-10)
        assert rc == want and (dec == 7.0).all() and (cf == 7.0).all(), (b, p)
