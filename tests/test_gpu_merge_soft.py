"""mbx_merge_detections_soft (Soft-NMS in the per-image merge, linear and gaussian), ImageMerger(soft=) and detect.py's
DETECTION.MERGE_SOFT_NMS, on the GPU.  Expected values come from tests/soft_oracle.py (numpy) or are hand-made.  Linear is
compared byte for byte.  Gaussian: on the five seeded cases the pick sequence is the oracle's (tests/test_soft_cpu.py
asserts the gap between unequal live scores that makes this legitimate) and scores are within 1 float32 ulp; everywhere
else the device's OWN pick sequence is replayed in the oracle and must be a best pick at every step within
delta(k) = 8 k 2^-53 (per pick both sides compute the same bits for -(o o) / sigma, each exp is within 1 ulp of the true
value, each side rounds one multiply: 6 * 2^-53 to first order, 8 leaves room for the second-order terms)."""
import json

import numpy as np
import pytest

from tests import soft_oracle as S
from tests.merge_oracle import CASES
from tests.test_gpu_merge import CFG, _detect_cmd, _run, cli_setup, lib, run_merge  # noqa: F401  (fixtures and helpers)
from tests.test_gpu_merge_vote import case_inputs  # noqa: F401  (fixture: the five seeded inputs)
from tests.vote_oracle import bound, vote_exact
from tests.vote_oracle import image_candidates as vote_candidates

pytestmark = pytest.mark.gpu
METHODS = {"linear": S.LINEAR, "gaussian": S.GAUSSIAN}
THR, SIGMA, MIN_SCORE = 0.3, 0.5, 0.001


def run_soft(lib, boxes, scores, count, image_rows, max_det, method, thr=THR, sigma=SIGMA, min_score=MIN_SCORE, vthr=0.0, votes=None):
    """One call; (rc, out_boxes, out_scores, out_src, out_count, out_status, out_votes) as numpy, pre-filled with 7.
    out_votes is passed iff vthr > 0, unless `votes` says otherwise."""
    import torch
    boxes, scores = np.ascontiguousarray(boxes, np.float64), np.ascontiguousarray(scores, np.float32)
    R, K = scores.shape
    assert boxes.shape == (R, K, 4) and len(count) == R and int(image_rows[-1]) <= R
    I = len(image_rows) - 1
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).cuda()
    d_b, d_s, d_c, d_r = dev(boxes, np.float64), dev(scores, np.float32), dev(count, np.int32), dev(image_rows, np.int32)
    n = max(I, 1)
    o_b = torch.full((n, max_det, 4), 7.0, dtype=torch.float64, device="cuda")
    o_s = torch.full((n, max_det), 7.0, dtype=torch.float32, device="cuda")
    o_i, o_v = (torch.full((n, max_det), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    o_c, o_st = (torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    with_votes = (vthr > 0) if votes is None else votes
    rc = lib.mbx_merge_detections_soft(d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), I, K, max_det, int(method),
                                       float(thr), float(sigma), float(min_score), float(vthr), o_b.data_ptr(), o_s.data_ptr(),
                                       o_i.data_ptr(), o_c.data_ptr(), o_st.data_ptr(), o_v.data_ptr() if with_votes else None,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (o_b, o_s, o_i, o_c, o_st, o_v))


def ulps32(a, b):
    """Distance in float32 steps between positive finite float32 arrays."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def same_bytes(x, y, fields=(1, 2, 3, 4, 5)):
    return all(x[j].tobytes() == y[j].tobytes() for j in fields)


def check_exact(lib, b, s, c, ir, max_det, method, exact_scores=True, **kw):
    """All outputs against the oracle's: byte for byte (linear), or the pick sequence exact and scores within 1 float32
    ulp (gaussian, where the caller knows the gap condition to hold); a second call gives the same bytes."""
    want = S.expected_arrays(b, S.soft_oracle(b, s, c, ir, max_det, method, kw.get("thr", THR), kw.get("sigma", SIGMA),
                                              kw.get("min_score", MIN_SCORE)), max_det)
    got, again = run_soft(lib, b, s, c, ir, max_det, method, **kw), run_soft(lib, b, s, c, ir, max_det, method, **kw)
    assert got[0] == 0 and again[0] == 0 and same_bytes(got, again)
    assert (got[6] == 7).all()                                            # no voting: out_votes is not touched
    eb, es, ei, ec, est = want
    print("picks", ec.tolist(), "device", got[4].tolist(), "status", got[5].tolist())
    assert np.array_equal(got[5], est) and np.array_equal(got[4], ec) and np.array_equal(got[3], ei)
    assert got[1].tobytes() == eb.tobytes()
    if exact_scores:
        assert got[2].tobytes() == es.tobytes()
    else:
        used = ei >= 0
        d = ulps32(got[2][used], es[used])
        print("scores: %d of %d differ, by at most %d float32 ulp" % (int((d > 0).sum()), d.size, int(d.max()) if d.size else 0))
        assert not got[2][~used].any() and (d <= 1).all()
    return got


def check_replay(lib, b, s, c, ir, max_det, sigma=SIGMA, min_score=MIN_SCORE, got=None):
    """Gaussian without a gap condition: the device's own pick sequence, replayed in the oracle."""
    got = run_soft(lib, b, s, c, ir, max_det, S.GAUSSIAN, sigma=sigma, min_score=min_score) if got is None else got
    rc, ob, os_, oi, oc, ost, ov = got
    assert rc == 0
    fb, fs, K = b.reshape(-1, 4), s.reshape(-1), s.shape[1]
    worst_pick, worst_stop, worst_ulp = 0.0, 0.0, 0
    for i in range(len(ir) - 1):
        flat = S.image_candidates(s, c, int(ir[i]), int(ir[i + 1]))
        nk = int(oc[i])
        if len(flat) > S.CAND_LIMIT:
            assert ost[i] == 1 and nk == 0 and (oi[i] == -1).all() and not ob[i].any() and not os_[i].any()
            continue
        assert ost[i] == 0 and 0 <= nk <= max_det
        assert (oi[i, nk:] == -1).all() and not ob[i, nk:].any() and not os_[i, nk:].any()       # unused slots
        src = oi[i, :nk].astype(np.int64)
        pos = np.searchsorted(flat, src)
        assert (pos < len(flat)).all() and np.array_equal(flat[np.minimum(pos, len(flat) - 1)], src) and len(set(src.tolist())) == nk
        assert ob[i, :nk].tobytes() == fb[src].tobytes()                  # the source's bytes
        t_pick, t_best, was_live, left = S.replay(fb[flat], fs[flat], pos, S.GAUSSIAN, 0.0, sigma, min_score)
        assert was_live.all()
        delta = 8.0 * np.arange(nk) * 2.0 ** -53
        assert (t_pick >= t_best * (1.0 - 2.0 * delta)).all(), (i, np.nonzero(t_pick < t_best * (1.0 - 2.0 * delta))[0][:5])
        miss = (t_best - t_pick) / t_best
        if nk > 1:
            worst_pick = max(worst_pick, float((miss[1:] / (2.0 * delta[1:])).max()))
        if nk < max_det:                                                  # stopped short: nobody may be live any more
            lim = min_score * (1.0 + 2.0 * 8.0 * nk * 2.0 ** -53)
            assert left <= lim, (i, left, lim)
            if left > min_score:
                worst_stop = max(worst_stop, (left / min_score - 1.0) / (2.0 * 8.0 * nk * 2.0 ** -53))
        d = ulps32(os_[i, :nk], t_pick.astype(np.float32))
        assert (d <= 1).all(), (i, int(d.max()))
        worst_ulp = max(worst_ulp, int(d.max()) if nk else 0)
        assert (np.diff(os_[i, :nk]) <= 0).all()
    print("replay: picks %s  worst (best - picked) / best / 2 delta %.3g  worst stop excess / 2 delta %.3g  worst score error %d "
          "float32 ulp" % (oc.tolist(), worst_pick, worst_stop, worst_ulp))
    return got


# the hand-made three of tests/test_soft_cpu.py: IoU(A, B) = 0.5 exactly, C apart
KNOWN = (np.array([[[0, 0, 2, 2], [0, 0, 2, 4], [10, 10, 12, 12]]], np.float64), np.array([[0.75, 0.5, 0.25]], np.float32),
         np.array([3], np.int32), np.array([0, 1], np.int32))


def test_known_answers(lib):
    b, s, c, ir = KNOWN
    f32 = lambda v: np.array(v, np.float32).tobytes()
    for thr, min_score, scores, src in ((0.3, 0.0, [0.75, 0.25, 0.25, 0], [0, 1, 2, -1]),          # B and C tie bit-equal: lower index
                                        (0.5, 0.0, [0.75, 0.5, 0.25, 0], [0, 1, 2, -1]),           # 0.5 is not > 0.5
                                        (0.3, 0.3, [0.75, 0, 0, 0], [0, -1, -1, -1])):
        rc, ob, os_, oi, oc, ost, ov = run_soft(lib, b, s, c, ir, 4, S.LINEAR, thr=thr, min_score=min_score)
        n = sum(x >= 0 for x in src)
        assert rc == 0 and oc.tolist() == [n] and ost.tolist() == [0] and oi[0].tolist() == src and os_[0].tobytes() == f32(scores)
        assert ob[0, :n].tobytes() == b[0, :n].tobytes() and not ob[0, n:].any() and (ov == 7).all()
    rc, ob, os_, oi, oc, ost, ov = run_soft(lib, b, s, c, ir, 4, S.GAUSSIAN, sigma=0.5, min_score=0.0)
    assert rc == 0 and oc.tolist() == [3] and oi[0].tolist() == [0, 1, 2, -1] and ob[0, :3].tobytes() == b[0].tobytes()
    assert os_[0, 0] == 0.75 and os_[0, 2] == 0.25 and os_[0, 3] == 0
    assert ulps32(os_[0, 1:2], np.array([0.5 * np.exp(-0.5)], np.float32))[0] <= 1 and os_[0, 1] > 0.25       # B ahead of C
    check_exact(lib, b, s, c, ir, 4, S.LINEAR, thr=0.3, min_score=0.0)


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_generator_cases(lib, case_inputs, name, method):
    """The five seeded cases x {linear 0.3, gaussian sigma 0.5}, min_score 0.001."""
    _, max_det, _ = CASES[name]
    b, s, c, ir = case_inputs[name]
    got = check_exact(lib, b, s, c, ir, max_det, METHODS[method], exact_scores=method == "linear")
    assert (np.diff(got[2], axis=1) <= 0).all()                           # non-increasing, the zeros of the unused slots included
    if method == "gaussian":
        check_replay(lib, b, s, c, ir, max_det, got=got)


@pytest.mark.parametrize("kw,max_det", [(dict(seed=31, I=5, rows_per_image=(2, 9), K=50, n_obj=4), 100),
                                        (dict(seed=32, I=3, rows_per_image=(30, 45), K=50, n_obj=9), 120)])
def test_gaussian_on_fresh_inputs_by_replay(lib, kw, max_det):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(**kw)
    got = check_replay(lib, b, s, c, ir, max_det)
    assert got[4].min() < max_det if kw["seed"] == 31 else got[4].min() == max_det       # both exits of the loop


# ------------------------------------------------------------------------------------------------------------------ edges
# the kernel's workgroup is 1 024 threads taking two candidates each per pass: the stride edges, and the wave's
EDGE_COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 0, 3000]


@pytest.fixture(scope="module")
def edge_input():
    """One image per entry of EDGE_COUNTS (rows of 300 slots, the last one partial; the image of 0 candidates has seven
    rows of count 0), and an image WITHOUT rows (r0 == r1) after the third."""
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=41, I=len(EDGE_COUNTS), rows_per_image=(10, 10), K=300, n_obj=6, count=0)
    for i, n in enumerate(EDGE_COUNTS):
        c[ir[i]:ir[i + 1]] = np.clip(n - 300 * np.arange(10), 0, 300)
    ir = np.concatenate([ir[:4], ir[3:]]).astype(np.int32)
    return b, s, c, ir


@pytest.mark.parametrize("method", sorted(METHODS))
def test_stride_edges_and_empty_images(lib, edge_input, method):
    b, s, c, ir = edge_input
    if method == "linear":
        got = check_exact(lib, b, s, c, ir, 24, S.LINEAR)
    else:
        got = check_replay(lib, b, s, c, ir, 24)
    oc = got[4]
    assert oc[0] == 1 and oc[3] == 0 and oc[11] == 0 and oc[12] == 24     # one candidate; no rows; rows of count 0; a full list
    for i in (3, 11):
        assert got[5][i] == 0 and (got[3][i] == -1).all() and not got[1][i].any() and not got[2][i].any()


@pytest.mark.parametrize("method", sorted(METHODS))
def test_an_image_does_not_depend_on_its_neighbours(lib, edge_input, method):
    """Every image of the mixed-size launch gives the bytes of that image launched alone."""
    b, s, c, ir = edge_input
    K = s.shape[1]
    full = run_soft(lib, b, s, c, ir, 24, METHODS[method])
    assert full[0] == 0
    for i in range(len(ir) - 1):
        a0, a1 = int(ir[i]), int(ir[i + 1])
        if a0 == a1:
            continue
        alone = run_soft(lib, b[a0:a1], s[a0:a1], c[a0:a1], np.array([0, a1 - a0], np.int32), 24, METHODS[method])
        assert alone[0] == 0
        for j in (1, 2, 4, 5):
            assert alone[j][0].tobytes() == full[j][i].tobytes(), (i, j)
        used = full[3][i] >= 0
        assert np.array_equal(alone[3][0] >= 0, used) and np.array_equal(alone[3][0][used], full[3][i][used] - a0 * K)


def test_clamped_counts_k_max_7_and_the_max_det_edges(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=42, I=2, rows_per_image=(3, 3), K=7, n_obj=2)
    s = np.maximum(s, np.float32(1 / 64))
    c = np.array([-3, 100, 7, 0, 2, 9], np.int32)                         # clamped to 0 7 7 | 0 2 7
    for method in METHODS.values():
        clamped = run_soft(lib, b, s, np.clip(c, 0, 7), ir, 20, method)
        got = run_soft(lib, b, s, c, ir, 20, method)
        assert got[0] == 0 and same_bytes(got, clamped)
    check_exact(lib, b, s, c, ir, 20, S.LINEAR)
    got = check_replay(lib, b, s, c, ir, 20)
    assert 2 <= got[4][0] <= 14 and 2 <= got[4][1] <= 9                   # 0 7 7 | 0 2 7 candidates
    # max_det 1: the best candidate, the lower flat index among equals
    for method in METHODS.values():
        rc, ob, os_, oi, oc, ost, ov = run_soft(lib, b, s, c, ir, 1, method)
        for i, flat in enumerate((S.image_candidates(s, c, 0, 3), S.image_candidates(s, c, 3, 6))):
            best = flat[np.argmax(s.reshape(-1)[flat])]
            assert rc == 0 and oc[i] == 1 and oi[i, 0] == best and os_[i, 0] == s.reshape(-1)[best]
    # max_det 640 with fewer candidates than that
    check_exact(lib, b, s, c, ir, 640, S.LINEAR)
    assert check_replay(lib, b, s, c, ir, 640)[4].tolist() == got[4].tolist()


@pytest.fixture(scope="module")
def limit_input():
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=12, I=3, rows_per_image=(82, 82), K=200, n_obj=30, count=200)
    c[:82] = 20                                                           # image 0: 1 640 candidates
    c[163] = 185                                                          # image 1: 81 * 200 + 185 = 16 385
    c[245] = 184                                                          # image 2: exactly 16 384
    return b, s, c, ir


@pytest.mark.parametrize("method", sorted(METHODS))
def test_candidate_limit_and_max_det_640(lib, limit_input, method):
    b, s, c, ir = limit_input
    if method == "linear":
        rc, ob, os_, oi, oc, ost, ov = check_exact(lib, b, s, c, ir, 640, S.LINEAR)
    else:
        rc, ob, os_, oi, oc, ost, ov = check_replay(lib, b, s, c, ir, 640)
    assert ost.tolist() == [0, 1, 0] and oc[1] == 0 and oc[2] == 640
    assert (oi[1] == -1).all() and not ob[1].any() and not os_[1].any()
    # the neighbours are what they are without image 1
    keep = np.r_[0:82, 164:246]
    two = run_soft(lib, b[keep], s[keep], c[keep], np.array([0, 82, 164], np.int32), 640, METHODS[method])
    for j, full in ((1, ob), (2, os_), (4, oc), (5, ost)):
        assert two[j][0].tobytes() == full[0].tobytes() and two[j][1].tobytes() == full[2].tobytes()


def test_who_never_comes_out(lib):
    """NaN, +-inf, +-0 and negative scores are never picked and decay nobody -- under a min_score of 0 too."""
    b = np.zeros((1, 8, 4))
    b[0] = [[0, 0, 10, 10 + 0.25 * k] for k in range(8)]                 # all overlap heavily
    s = np.array([[0.25, np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 0.5]], np.float32)
    c, ir = np.array([8], np.int32), np.array([0, 1], np.int32)
    for min_score in (0.0, 0.001):
        rc, ob, os_, oi, oc, ost, ov = check_exact(lib, b, s, c, ir, 8, S.LINEAR, thr=0.3, min_score=min_score)
        assert oc[0] == 2 and oi[0, :2].tolist() == [7, 0] and os_[0, 0] == 0.5
        # 0.25 was decayed by the pick 0.5 alone: IoU of [0,0,10,11.75] and [0,0,10,10] is 100 / 117.5
        assert os_[0, 1] == np.float32(0.25 * (1.0 - 100.0 / 117.5))
        got = check_replay(lib, b, s, c, ir, 8, min_score=min_score)
        assert got[4][0] == 2 and got[3][0, :2].tolist() == [7, 0]


def test_equal_scores_on_disjoint_boxes_come_out_in_flat_index_order(lib):
    n = 150                                                               # three wavefronts' worth, over two rows of 100 slots
    b = np.zeros((2, 100, 4))
    b.reshape(-1, 4)[:n] = [[k, 0, k + 0.5, 1] for k in range(n)]
    s = np.zeros((2, 100), np.float32)
    s.reshape(-1)[:n] = 0.5
    c, ir = np.array([100, 50], np.int32), np.array([0, 2], np.int32)
    for method in METHODS.values():                                       # weights are exactly 1 under both methods
        rc, ob, os_, oi, oc, ost, ov = check_exact(lib, b, s, c, ir, 160, method)
        assert oc[0] == n and oi[0, :n].tolist() == list(range(n)) and (os_[0, :n] == 0.5).all()


def test_unsorted_rows_give_the_same_result(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=8, I=3, rows_per_image=(5, 12), K=40, n_obj=4, count=40)
    rng = np.random.RandomState(0)
    s = ((1 + rng.permutation(s.size)).astype(np.float32) / np.float32(s.size)).reshape(s.shape)      # distinct scores
    srt = np.argsort(-s, axis=1, kind="stable")
    bs, ss = np.take_along_axis(b, srt[:, :, None], 1), np.take_along_axis(s, srt, 1)
    perm = np.stack([rng.permutation(40) for _ in range(len(c))])
    bu, su = np.take_along_axis(bs, perm[:, :, None], 1), np.take_along_axis(ss, perm, 1)
    check_exact(lib, bu, su, c, ir, 30, S.LINEAR)
    for method in METHODS.values():
        a, u = run_soft(lib, bs, ss, c, ir, 30, method), run_soft(lib, bu, su, c, ir, 30, method)
        assert a[0] == 0 and u[0] == 0 and same_bytes(a, u, fields=(1, 2, 4, 5))


# ------------------------------------------------------------------------------------------- against the existing kernels
def test_linear_at_threshold_one_is_the_plain_top_n(lib, case_inputs):
    """Nothing decays (no IoU is > 1) and with min_score 0 every positive finite score is live: mbx_merge_detections at +inf."""
    for name in ("topn", "small"):
        _, max_det, _ = CASES[name]
        b, s, c, ir = case_inputs[name]
        s = s + np.float32(1 / 64)                                        # positive, ties kept
        plain = run_merge(lib, b, s, c, ir, max_det, np.inf)
        soft = run_soft(lib, b, s, c, ir, max_det, S.LINEAR, thr=1.0, min_score=0.0)
        assert plain[0] == 0 and soft[0] == 0
        for j in range(1, 6):
            assert soft[j].tobytes() == plain[j].tobytes(), (name, j)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_voting_behind_soft_nms(lib, case_inputs, method):
    """vote_iou_threshold 0.6: scores, sources and counts are the unvoted soft call's bytes, the votes are the oracle's
    count of voters around every pick (weights: the ORIGINAL scores), the boxes are within the voting bound."""
    from fractions import Fraction
    _, max_det, _ = CASES["typical"]
    b, s, c, ir = case_inputs["typical"]
    unvoted = run_soft(lib, b, s, c, ir, max_det, METHODS[method])
    got, again = (run_soft(lib, b, s, c, ir, max_det, METHODS[method], vthr=0.6) for _ in range(2))
    assert unvoted[0] == 0 and got[0] == 0 and same_bytes(got, again, fields=(1, 2, 3, 4, 5, 6))
    assert same_bytes(got, unvoted, fields=(2, 3, 4, 5)) and got[1].tobytes() != unvoted[1].tobytes()
    rc, ob, os_, oi, oc, ost, ov = got
    fb, fs, worst, moved = b.reshape(-1, 4), s.reshape(-1), Fraction(0), 0
    for i in range(len(ir) - 1):
        nk = int(oc[i])
        assert not ov[i, nk:].any() and not ob[i, nk:].any()
        src = oi[i, :nk].astype(np.int64)
        cand = vote_candidates(s, c, int(ir[i]), int(ir[i + 1]))
        mean, absmean, n = vote_exact(fb[src], fb[cand], fs[cand], 0.6)
        assert np.array_equal(ov[i, :nk], n) and n.max() > 1
        for k in range(nk):
            if n[k] == 0:
                assert ob[i, k].tobytes() == fb[src[k]].tobytes()
                continue
            for j in range(4):
                err, lim = abs(Fraction(float(ob[i, k, j])) - mean[k][j]), bound(n[k], absmean[k][j])
                assert err <= lim, (i, k, j, float(err), float(lim))
                worst = max(worst, err / lim) if lim > 0 else worst
    print("votes behind %s soft-NMS: worst error / bound %.3g" % (method, float(worst)))


def test_bad_arguments(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=7, I=2, rows_per_image=(2, 2), K=10, n_obj=2, count=10)
    untouched = lambda got: all((x == 7).all() for x in got[1:])
    nan, inf = float("nan"), float("inf")
    bad = [dict(method=0), dict(method=3), dict(method=-1),
           dict(method=S.LINEAR, thr=nan),
           dict(method=S.GAUSSIAN, sigma=0.0), dict(method=S.GAUSSIAN, sigma=-0.5), dict(method=S.GAUSSIAN, sigma=nan),
           dict(method=S.GAUSSIAN, sigma=inf)]
    for method in METHODS.values():
        bad += [dict(method=method, min_score=v) for v in (nan, -0.001, inf, -inf)]
        bad += [dict(method=method, vthr=v, votes=True) for v in (nan, -0.1, 1.5, float(np.nextafter(1.0, 2)), inf, -inf)]
        bad += [dict(method=method, vthr=0.6, votes=False)]               # voting asked for, null out_votes
    for kw in bad:
        got = run_soft(lib, b, s, c, ir, 5, **kw)
        assert got[0] == -1 and untouched(got), kw
    for method in METHODS.values():
        got = run_soft(lib, b, s, c, ir, 641, method)
        assert got[0] == -2 and untouched(got)
        got = run_soft(lib, b, s, c, np.array([0], np.int32), 5, method)                       # I == 0: nothing launched
        assert got[0] == 0 and untouched(got)
    # what the other method's parameter holds does not matter; the limits of the ranges are accepted
    assert run_soft(lib, b, s, c, ir, 5, S.LINEAR, thr=0.3, sigma=nan)[0] == 0
    assert run_soft(lib, b, s, c, ir, 5, S.GAUSSIAN, thr=nan, sigma=0.5)[0] == 0
    assert run_soft(lib, b, s, c, ir, 640, S.LINEAR, thr=inf, min_score=0.0, vthr=1.0)[0] == 0
    assert run_soft(lib, b, s, c, ir, 5, S.LINEAR, thr=-inf, vthr=0.0, votes=True)[0] == 0     # no voting: out_votes is ignored
    import torch
    p = torch.zeros(64, dtype=torch.float64, device="cuda").data_ptr()
    call = lambda **kw: lib.mbx_merge_detections_soft(*[kw.get(k, d) for k, d in (
        ("boxes", p), ("scores", p), ("count", p), ("rows", p), ("I", 1), ("k_max", 1), ("max_det", 1), ("method", 1), ("thr", 0.5),
        ("sigma", 0.5), ("min_score", 0.001), ("vthr", 0.5), ("ob", p), ("os", p), ("oi", p), ("oc", p), ("ost", p), ("ov", p),
        ("stream", None))])
    for name in ("boxes", "scores", "count", "rows", "ob", "os", "oi", "oc", "ost", "ov"):
        assert call(**{name: None}) == -1, name
    assert call(k_max=0) == -1 and call(max_det=0) == -1 and call(I=-1) == -1 and call(I=0) == 0
    assert call(ov=None, vthr=0.0, I=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ ImageMerger
@pytest.mark.parametrize("batch,flush_images", [(4, 1), (64, 1), (4, 256), (64, 256)])
def test_image_merger_soft_like_one_call(lib, case_inputs, batch, flush_images):
    from multibox_amd.detect import ImageMerger
    _, max_det, thr = CASES["typical"]
    b, s, c, ir = case_inputs["typical"]
    ids = [100 + i for i in range(len(ir) - 1) for _ in range(ir[i + 1] - ir[i])]

    def feed(iou=thr, **kw):
        m = ImageMerger(b.shape[1], max_det, iou, flush_images=flush_images, **kw)
        for a in range(0, len(c), batch):
            m.add(b[a:a + batch], s[a:a + batch], c[a:a + batch], ids[a:a + batch])
        return m.finish()
    for soft, iou, vote, direct in ((("gaussian", 0.25, 0.002), None, None, dict(method=S.GAUSSIAN, sigma=0.25, min_score=0.002)),
                                    (("linear", 0.5, 0.001), 0.3, 0.6, dict(method=S.LINEAR, thr=0.3, vthr=0.6))):
        rc, ob, os_, oi, oc, ost, ov = run_soft(lib, b, s, c, ir, max_det, **direct)
        got_ids, gb, gs, gc = feed(iou=iou, soft=soft, vote_iou=vote)
        assert rc == 0 and got_ids == [100 + i for i in range(len(ir) - 1)]
        assert gb.tobytes() == ob.tobytes() and gs.tobytes() == os_.tobytes() and np.array_equal(gc, oc)
    plain = run_merge(lib, b, s, c, ir, max_det, thr)
    got_ids, gb, gs, gc = feed(soft=None)                                 # off: today's bytes
    assert gb.tobytes() == plain[1].tobytes() and gs.tobytes() == plain[2].tobytes() and np.array_equal(gc, plain[4])
    assert gs.tobytes() != os_.tobytes()
    with pytest.raises(ValueError):
        ImageMerger(b.shape[1], max_det, None, soft=("linear", 0.5, 0.001))


def test_image_merger_cuts_an_oversize_image_on_the_host_then_soft_merges(lib, capsys):
    from multibox_amd import records as REC
    from multibox_amd.detect import ImageMerger
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=13, I=3, rows_per_image=(90, 90), K=200, n_obj=12, count=200)
    c[:90], c[180:] = 10, 25                                              # images 0 and 2 small, image 1: 18 000 candidates
    ids = ["a"] * 90 + ["b"] * 90 + ["c"] * 90
    m = ImageMerger(200, 100, 0.3, flush_images=2, soft=("linear", 0.5, 0.001))
    for a in range(0, len(c), 64):
        m.add(b[a:a + 64], s[a:a + 64], c[a:a + 64], ids[a:a + 64])
    got_ids, gb, gs, gc = m.finish()
    assert got_ids == ["a", "b", "c"] and capsys.readouterr().out.count("WARNING") == 1
    # the oracle on the same cut: image 1's best 16 384 in merge order, as fresh rows
    cut = REC.repack_rows(b[90:180], s[90:180], REC.best_candidates(s[90:180], c[90:180]), 200)
    assert int(cut[2].sum()) == 16384
    for i, (bb, ss, cc) in enumerate(((b[:90], s[:90], c[:90]), cut, (b[180:], s[180:], c[180:]))):
        eb, es, ei, ec, est = S.expected_arrays(bb, S.soft_oracle(bb, ss, cc, np.array([0, len(cc)]), 100, S.LINEAR, 0.3, 0.5, 0.001), 100)
        assert gc[i] == ec[0] and gb[i].tobytes() == eb[0].tobytes() and gs[i].tobytes() == es[0].tobytes(), i
    assert gc[1] == 100


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_soft_nms_key(cli_setup):
    """detect.py --merge_per_image with DETECTION.MERGE_SOFT_NMS gaussian, null and absent."""
    d = cli_setup
    (d / "config_soft.yaml").write_text(CFG + "  MERGE_SOFT_NMS : gaussian\n")
    (d / "config_soft_null.yaml").write_text(CFG + "  MERGE_SOFT_NMS : null\n")
    _run(_detect_cmd(d, "merged", "--merge_per_image", "--max_detections", "20"))
    for cfg, out in (("config_soft.yaml", "soft"), ("config_soft_null.yaml", "soft_null")):
        cmd = _detect_cmd(d, out, "--merge_per_image", "--max_detections", "20")
        cmd[cmd.index("--config") + 1] = str(d / cfg)
        _run(cmd)
    read = lambda out, name: open(d / out / name, "rb").read()
    assert read("soft", "results-dense-0.json") == read("merged", "results-dense-0.json")
    assert read("soft_null", "results-merged-0.json") == read("merged", "results-merged-0.json")
    plain, soft = (json.loads(read(n, "results-merged-0.json")) for n in ("merged", "soft"))
    per_image = {}
    for x in soft:
        per_image.setdefault(x["image_id"], []).append(x["score"])
    assert sorted(per_image) == [1000, 1001, 1002]
    for image_id, sc in per_image.items():
        assert len(sc) <= 20 and all(u >= v for u, v in zip(sc, sc[1:])), image_id
    print("merged records: greedy %d, soft %d" % (len(plain), len(soft)))
    assert [(x["image_id"], x["score"]) for x in plain] != [(x["image_id"], x["score"]) for x in soft]
