"""tests/postproc_oracle.py on the CPU: the oracle's own helpers, and the preconditions every case of
tests/test_gpu_postproc_edges.py relies on, proved on the reference alone -- real ties in the tie inputs and scipy optimal on
them, gaps in the tie-free inputs, bit-exact boundary coordinates, an IoU of exactly 0.5, the launch-shape boundaries
re-derived from the host's formulas."""
import math

import numpy as np
import pytest

from oracle import ref_numpy as R
from tests import postproc_oracle as O


@pytest.fixture(scope="module")
def tie_cases(golden):
    return O.match_tie_cases(golden.priors["k5_restrict"])


# ------------------------------------------------------------------------------------------------------------ helpers
def test_assignment_cost_checks_validity():
    C = np.arange(12, dtype=np.float64).reshape(4, 3)                    # P = 4, n = 3
    assert O.assignment_cost(C, [0, -1, 2, 1]) == C[0, 0] + C[2, 2] + C[3, 1]
    for bad in ([0, 0, 2, 1], [0, -1, -1, 1], [0, -2, 2, 1], [0, 3, 2, 1], [0, 1, 2]):
        with pytest.raises(AssertionError):
            O.assignment_cost(C, bad)
    assert O.assignment_cost(np.zeros((4, 0)), [-1] * 4) == 0.0
    big = np.array([[1e16, 1.0], [1.0, -1e16], [1.0, 1.0]])              # fsum: no rounding of its own
    assert O.assignment_cost(big, [0, 1, -1]) == 0.0 and O.assignment_cost(big, [0, -1, 1]) == 1e16 + 1.0


def test_bruteforce_and_margin_on_known_matrices():
    C = np.array([[4.0, 1.0], [2.0, 0.0], [3.0, 2.0]])
    assert O.lsap_bruteforce(C) == 3.0 == O.scipy_total(C)               # (1, 0) + (0, 1) or (0,1)+(1,0): 2 + 1
    assert O.second_best_margin(np.array([[0.0, 5.0], [5.0, 0.0]])) == 10.0
    assert O.second_best_margin(np.zeros((3, 2))) == 0.0
    assert O.min_gap_ulps(np.array([[1.0, 1.0 + 2.0 ** -20], [3.0, 2.0]])) == pytest.approx(2.0 ** -20 / O.ulp32(3.0))
    assert O.min_gap_ulps(np.array([[1.0, 2.0], [3.0, 2.0]])) == 0.0 and O.min_gap_ulps(np.ones((1, 1))) == np.inf


def test_cost_matrix_restatement_is_byte_identical():
    for kind in ("plain", "conf_one", "far_one"):
        dec, conf, gt = O.match_special_case(kind)
        with np.errstate(over="ignore", invalid="ignore"):
            assert O.cost_matrix_lastbit(dec, conf, gt, 1000.0).tobytes() == O.costs(dec, conf, gt, len(gt), 1000.0).tobytes()
    moved = O.cost_matrix_lastbit(*O.match_special_case("plain"), 1.0, np.random.RandomState(0))     # alpha 1: costs near the logs
    C = O.costs(*O.match_special_case("plain"), 5, 1.0)
    assert (moved != C).any() and np.abs(moved - C).max() <= 4 * O.ulp32(np.abs(C).max())


def test_sigmoid_ref_special_values():
    z = np.array([0.0, np.inf, -np.inf, -200.0, np.nan, 1.0], np.float32)
    for eps in (np.float32(1e-10), np.float32(0.0)):
        s = O.sigmoid_ref(z, eps)
        assert s.dtype == np.float32
        assert s[0] == np.float32(0.5) and s[1] == np.float32(1.0) and s[2] == eps and s[3] == eps and np.isnan(s[4])
        assert abs(float(s[5]) - 1.0 / (1.0 + math.exp(-1.0))) <= O.ulp32(0.73)


# ------------------------------------------------------------------------------------------------------ launch shapes
def test_launch_shape_boundaries_follow_the_host_formulas():
    shapes = set(O.MATCH_SHAPES)
    P64 = max(P for P in range(1, 5000) if O.match_lds_bytes(P, 16) <= 64 * 1024)
    assert (2, P64, 16) in shapes and (2, P64 + 1, 16) in shapes and (P64, P64 + 1) == (1812, 1813)
    Pmax = max(P for P in range(1, 5000) if O.match_lds_bytes(P, 100) <= 150 * 1024)
    assert (2, Pmax, 100) in shapes and O.MATCH_TOO_BIG == (1, Pmax + 1, 100) and Pmax == 4221
    assert (3, 1536, 20) in shapes and (3, 1537, 20) in shapes                     # nthreads = P > 1536 ? 512 : 256
    lo, hi = O.nms_lds_crossing()
    assert (lo, hi) == (704, 705) and O.nms_lds_bytes(lo) <= 65536 < O.nms_lds_bytes(hi) <= 160 * 1024
    assert O.nms_lds_bytes(1024) == (1024 * 16 + 16) * 8 <= 160 * 1024


# ---------------------------------------------------------------------------------------------------- mbx_match inputs
@pytest.mark.parametrize("B,P,G", O.MATCH_SHAPES)
def test_launch_cases_are_tie_free(B, P, G):
    dec, conf, gt, n = O.match_launch_case(B, P, G)
    assert n[0] == min(G, P) and (B == 1 or n[1] == 0) and (n <= min(G, P)).all()
    again = O.match_launch_case(B, P, G)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((dec, conf, gt, n), again))       # the seed is fixed
    for b in range(B):
        assert not gt[b, n[b]:].any()
        if n[b] > 0:
            gap = O.min_gap_ulps(O.costs(dec[b], conf[b], gt[b], n[b], 1000.0))
            print("P %d n %d: smallest gap %.1f ulps" % (P, n[b], gap))
            assert gap > O.GAP_ULPS


@pytest.mark.parametrize("kind", ["plain", "conf_one", "far_one"])
def test_special_cases_are_tie_free_and_scipy_takes_them(kind):
    dec, conf, gt = O.match_special_case(kind)
    C = O.costs(dec, conf, gt, len(gt), 1000.0)
    assert O.min_gap_ulps(C) > O.GAP_ULPS
    _, _, m = R.compute_assignments(dec, conf, gt[None], [len(gt)], 1, 1000.0) if kind != "far_one" else (0, 0, None)
    if kind == "conf_one":
        assert conf[3] == 1.0 and conf[17] == 1.5 and m[0, 3] >= 0 and m[0, 17] >= 0
    if kind == "far_one":
        assert np.isposinf(C[11]).all() and np.isfinite(np.delete(C, 11, 0)).all()
        with np.errstate(over="ignore"):
            _, _, m = R.compute_assignments(dec, conf, gt[None], [len(gt)], 1, 1000.0)
        assert m[0, 11] == -1 and O.assignment_cost(C, m[0]) == O.scipy_total(C)


def test_every_prediction_far_is_infeasible_for_scipy():
    dec, conf, gt = O.match_special_case("far_all")
    assert np.isposinf(O.costs(dec, conf, gt, len(gt), 1000.0)).all()
    with pytest.raises(ValueError), np.errstate(over="ignore"):
        R.compute_assignments(dec, conf, gt[None], [len(gt)], 1, 1000.0)


@pytest.mark.parametrize("alpha", [1000.0, 1e-3])
def test_contention_cases_do_not_depend_on_the_last_bit_of_log(alpha):
    dec, conf, gt, n, seed = O.match_contention_case(alpha)
    assert dec.shape == (1, 646, 4) and n.tolist() == [100]
    assert np.ptp(gt[0], axis=0).max() <= 0.01                            # inside a 0.01 neighbourhood of one box
    assert O.robust_to_log_lastbit(dec[0], conf[0], gt[0], alpha)
    C = O.costs(dec[0], conf[0], gt[0], 100, alpha)
    order = np.argsort(C, axis=0)[:100]                                    # every gt wants the same predictions
    assert len(set(order.ravel().tolist())) < 200
    if alpha < 1.0:
        assert len(set(order[:20].ravel().tolist())) < 40
    print("alpha %g seed %d: second best assignment worse by %.3g" % (alpha, seed, O.second_best_margin(C)))


def test_tie_cases_have_ties_and_scipy_is_optimal(tie_cases):
    assert sorted(tie_cases) == ["all_equal", "contention_flat", "start_of_training", "twin_gt", "twin_predictions"]
    for name, (dec, conf, gt, alpha) in tie_cases.items():
        n = len(gt)
        C = O.costs(dec, conf, gt, n, alpha)
        assert np.isfinite(C).all() and O.min_gap_ulps(C) == 0.0, name                    # equal entries in a row or a column
        if n > 6:
            continue
        if name == "all_equal":
            assert (C == C[0, 0]).all()
            small = C[:8]                                                 # every prediction is the same one: 8 of them do
        else:
            small = O.reduce_for_bruteforce(C)
        best = O.lsap_bruteforce(small)
        got = O.scipy_total(C)
        print("%s: %s reduced to %s, optimum %.17g, scipy %.17g" % (name, C.shape, small.shape, best, got))
        assert abs(got - best) <= 1e-12 * max(1.0, abs(best)), name       # float64 rounding of n entries, nothing more
    dec, conf, gt, _ = tie_cases["twin_gt"]
    assert gt[4].tobytes() == gt[1].tobytes() and dec.shape == (8, 4) and len(gt) == 6
    dec, conf, gt, _ = tie_cases["twin_predictions"]
    C = O.costs(dec, conf, gt, 3, 1000.0)
    twins = np.nonzero((C == C[3]).all(axis=1))[0]
    assert len(twins) == 8 and (np.delete(C, twins, 0).min(axis=0) > C[3]).all()            # 8 equal rows, the cheapest for all 3
    dec, conf, gt, _ = tie_cases["start_of_training"]
    flipped = np.stack([1 - gt[:, 2], 1 - gt[:, 3], 1 - gt[:, 0], 1 - gt[:, 1]], 1)           # the point reflection in the centre
    assert sorted(map(tuple, flipped)) == sorted(map(tuple, gt))
    assert len(set(conf.tolist())) == 1 and dec.shape == (646, 4)
    assert O.second_best_margin(O.costs(dec, conf, gt, 4, 1000.0)) == 0.0                    # more than one optimum


# ------------------------------------------------------------------------------------------ mbx_decode_filter_topk inputs
def test_boundary_case_decodes_to_the_exact_bits():
    raw, conf, priors, meta, target = O.topk_boundary_case()
    dec = (raw + priors[None]).astype(np.float32)                          # the kernel's float32 add
    assert dec.tobytes() == target.tobytes()
    res = O.BOUNDARY_RES
    assert res.dtype == np.float32 and (meta["res"] == res).all()
    as_int = lambda a: np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    step = np.array([-1, -1, 1, 1])                                        # in bit patterns (all positive): outward
    for g, want in enumerate((0, 1, -1)):                                  # equal, one ulp outside, one ulp inside
        for k in range(4):
            assert as_int(dec[g, k, k]) - as_int(res[k]) == want * step[k], (g, k)
            others = np.delete(np.arange(4), k)
            assert (np.abs(dec[g, k, others] - res[others]) > 0.01).all()
        assert np.array_equal(as_int(dec[g, 4]) - as_int(res), want * step)
        assert R.filter_mask(dec[g, 5:], res).all()
    assert R.filter_mask(dec[0], res).all() and R.filter_mask(dec[2], res).all()
    assert R.filter_mask(dec[1], res).tolist() == [False] * 5 + [True] * 4
    assert O.topk_expected(raw, conf, priors, meta, 16)[3].tolist() == [9, 4, 9]


def test_topk_expected_clamps_and_fills():
    raw, conf, priors, meta = O.topk_random_case(6, 65, 3)
    meta["mtk"][:] = [-3, 0, 1, 6, 7, 57]
    eb, es, ei, ec = O.topk_expected(raw, conf, priors, meta, 7)
    kept = [int(R.filter_mask(R.decode_clip(raw[b], priors), meta["res"][b]).sum()) for b in range(6)]
    assert min(kept) > 7 and ec.tolist() == [0, 0, 1, 6, 7, 7]
    for b in range(6):
        assert not eb[b, ec[b]:].any() and not es[b, ec[b]:].any() and (ei[b, ec[b]:] == -1).all() and (ei[b, :ec[b]] >= 0).all()
    conf[:] = 0.25                                                         # equal scores: the higher prediction index first
    ei = O.topk_expected(raw, conf, priors, meta, 7)[2]
    assert (np.diff(ei[4]) < 0).all()


# ------------------------------------------------------------------------------------------------------ mbx_nms inputs
def test_iou_exactly_at_the_threshold():
    b = np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 0.5]])
    iw, ih = min(b[0, 2], b[1, 2]) - max(b[0, 0], b[1, 0]), min(b[0, 3], b[1, 3]) - max(b[0, 1], b[1, 1])
    inter = iw * ih
    union = (b[0, 2] - b[0, 0]) * (b[0, 3] - b[0, 1]) + (b[1, 2] - b[1, 0]) * (b[1, 3] - b[1, 1]) - inter
    assert inter / union == 0.5                                            # nms_greedy's operation order, float64
    assert R.nms_greedy(b, 0.5).tolist() == [0, 1] and R.nms_greedy(b, np.nextafter(0.5, 0.0)).tolist() == [0]


def test_chain_gives_the_alternating_pattern():
    b = O.nms_boxes("chain", 300)
    iou = lambda i, j: (1.0 - (j - i) * 0.25) / (1.0 + (j - i) * 0.25)
    assert iou(0, 1) == 0.6 > 0.5 > iou(0, 2) > 0.0 and iou(0, 4) == 0.0
    assert R.nms_greedy(b, 0.5).tolist() == list(range(0, 300, 2))        # pairs (2k, 2k+1): across every 64 and 256 boundary
    assert R.nms_greedy(b, 0.0).tolist() == list(range(0, 300, 4))
    assert R.nms_greedy(b, 1.0).tolist() == list(range(300))


@pytest.mark.parametrize("pattern", O.NMS_PATTERNS)
def test_vectorised_greedy_equals_nms_greedy(pattern):
    for K in (1, 2, 64, 65, 130) + ((300,) if pattern == "last_sweep" else ()):
        b = O.nms_boxes(pattern, K)
        assert b.shape == (K, 4) and b.dtype == np.float64
        for thr in O.NMS_THRESHOLDS + (0.3,):
            assert np.array_equal(O.nms_greedy_vec(b, thr), R.nms_greedy(b, thr)), (K, thr)
    keep = O.nms_greedy_vec(O.nms_boxes("last_sweep", 1024), 0.5)
    assert keep[0] == 0 and keep[1] == 768 and len(keep) == 257            # the survivors but box 0 lie in the last sweep
    assert 10 < len(O.nms_greedy_vec(O.nms_boxes("clustered", 512), 0.5)) < 500
