"""mbx_merge_detections_wbf (weighted boxes fusion in the per-image merge), ImageMerger(wbf=) and detect.py's
DETECTION.MERGE_WBF, on the GPU.  Expected values come from tests/wbf_oracle.py (numpy) or are hand-made
(tests/test_wbf_cpu.py derives the numbers).  Every comparison is byte for byte on all six outputs, and a second call
must give the same bytes.  The kernel keeps the state of an image's first 320 clusters in LDS and the rest in the
workspace: the seeded cases `wide` (2 035 clusters) and the all-disjoint images of 319 / 320 / 321 cross that bound."""
import json

import numpy as np
import pytest

from tests import wbf_oracle as W
from tests.merge_oracle import CASES
from tests.test_gpu_merge import CFG, _detect_cmd, _run, cli_setup, lib, run_merge  # noqa: F401  (fixtures and helpers)
from tests.test_gpu_merge_vote import case_inputs  # noqa: F401  (fixture: the five seeded inputs)

pytestmark = pytest.mark.gpu
CONF = {"avg": W.AVG, "max": W.MAX}
LDS_CLUSTERS = 320


def run_wbf(lib, boxes, scores, count, image_rows, max_det, conf, thr=0.55, min_score=0.0, views=1, ws_bytes=None, R=None):
    """One call; (rc, out_boxes, out_scores, out_src, out_count, out_status, out_votes) as numpy, pre-filled with 7.  The
    workspace is handed over full of 0xa5 bytes: what it holds before the call must not matter."""
    import torch
    boxes, scores = np.ascontiguousarray(boxes, np.float64), np.ascontiguousarray(scores, np.float32)
    rows, K = scores.shape
    assert boxes.shape == (rows, K, 4) and len(count) == rows and int(image_rows[-1]) <= rows
    I = len(image_rows) - 1
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).cuda()
    d_b, d_s, d_c, d_r = dev(boxes, np.float64), dev(scores, np.float32), dev(count, np.int32), dev(image_rows, np.int32)
    n = max(I, 1)
    o_b = torch.full((n, max_det, 4), 7.0, dtype=torch.float64, device="cuda")
    o_s = torch.full((n, max_det), 7.0, dtype=torch.float32, device="cuda")
    o_i, o_v = (torch.full((n, max_det), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    o_c, o_st = (torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    need = lib.mbx_merge_wbf_workspace(rows, K)
    assert need == rows * K * 88
    ws = torch.full((need,), 0xa5, dtype=torch.uint8, device="cuda")
    rc = lib.mbx_merge_detections_wbf(d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), rows if R is None else R, I,
                                      K, max_det, int(conf), float(thr), float(min_score), int(views), o_b.data_ptr(),
                                      o_s.data_ptr(), o_i.data_ptr(), o_c.data_ptr(), o_st.data_ptr(), o_v.data_ptr(),
                                      ws.data_ptr(), need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (o_b, o_s, o_i, o_c, o_st, o_v))


def same_bytes(x, y, fields=(1, 2, 3, 4, 5, 6)):
    return all(x[j].tobytes() == y[j].tobytes() for j in fields)


def check_exact(lib, b, s, c, ir, max_det, conf, **kw):
    """All six outputs against the oracle's, byte for byte; a second call gives the same bytes."""
    res = W.wbf_oracle(b, s, c, ir, conf, kw.get("thr", 0.55), kw.get("min_score", 0.0), kw.get("views", 1))
    want = W.expected_arrays(res, max_det)
    got, again = run_wbf(lib, b, s, c, ir, max_det, conf, **kw), run_wbf(lib, b, s, c, ir, max_det, conf, **kw)
    assert got[0] == 0 and again[0] == 0 and same_bytes(got, again)
    print("clusters", [len(r[1]) for r in res], "device count", got[4].tolist(), "status", got[5].tolist())
    for j, name in enumerate(("boxes", "scores", "src", "count", "status", "votes")):
        assert got[j + 1].tobytes() == want[j].tobytes(), name
    return got, res


# ------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("thr", [0.55, 0.3])
@pytest.mark.parametrize("conf", sorted(CONF))
@pytest.mark.parametrize("name", sorted(CASES))
def test_generator_cases(lib, case_inputs, name, conf, thr):
    _, max_det, _ = CASES[name]
    b, s, c, ir = case_inputs[name]
    got, res = check_exact(lib, b, s, c, ir, max_det, CONF[conf], thr=thr, views=2 if conf == "max" else 1)
    assert (np.diff(got[2], axis=1) <= 0).all()                           # non-increasing, the zeros of the unused slots included
    if name == "wide" and thr == 0.55:
        assert max(len(r[1]) for r in res) > 4 * LDS_CLUSTERS - 64        # clusters far past what LDS holds


def test_known_answers(lib):
    """The hand-worked answers of tests/test_wbf_cpu.py."""
    def one(boxes, scores, conf, thr, views=1, max_det=4):
        b, s = np.array([boxes], np.float64), np.array([scores], np.float32)
        rc, ob, os_, oi, oc, ost, ov = run_wbf(lib, b, s, np.array([len(scores)], np.int32), np.array([0, 1], np.int32), max_det,
                                               conf, thr=thr, views=views)
        n = int(oc[0])
        assert rc == 0 and ost[0] == 0 and not ob[0, n:].any() and not os_[0, n:].any() and (oi[0, n:] == -1).all() and not ov[0, n:].any()
        return ob[0, :n].tolist(), os_[0, :n].tolist(), oi[0, :n].tolist(), ov[0, :n].tolist()
    half, scores = [[0, 0, 2, 1], [0, 0, 1, 1]], [0.75, 0.25]
    below = float(np.nextafter(0.5, 0.0))
    assert one(half, scores, W.AVG, 0.5) == ([[0, 0, 2, 1], [0, 0, 1, 1]], [0.75, 0.25], [0, 1], [1, 1])      # IoU 1/2 is not > 0.5
    assert one(half, scores, W.AVG, below) == ([[0, 0, 1.75, 1]], [0.5], [0], [2])
    assert one(half, scores, W.MAX, below) == ([[0, 0, 1.75, 1]], [0.75], [0], [2])
    between, scores = [[0, 0, 2, 2], [2, 0, 4, 2], [1, 0, 3, 2]], [0.75, 0.5, 0.25]
    assert one(between, scores, W.AVG, 0.3) == ([[0.25, 0, 2.25, 2], [2, 0, 4, 2]], [0.5, 0.5], [0, 1], [2, 1])   # IoU 1/3 with both: the lower
    assert one(between, scores, W.AVG, 0.34)[3] == [1, 1, 1]
    chain, scores = [[0, 0, 4, 4], [2, 0, 6, 4], [3, 0, 7, 4]], [0.5, 0.5, 0.25]
    want = [1.75 / 1.25, 0.0, 6.75 / 1.25, 5.0 / 1.25]                    # C matches the fused box of A and B (1/3), not A (1/7)
    assert one(chain, scores, W.AVG, 0.3) == ([want], [float(np.float32(1.25 / 3.0))], [0], [3])
    views = [[0, 0, 1, 1]] + [[2, 0, 3, 1]] * 2 + [[4, 0, 5, 1]] * 6
    scores = [0.5] + [0.75, 0.25] + [0.5, 0.25, 0.25, 0.25, 0.125, 0.125]
    assert one(views, scores, W.MAX, 0.55, views=5)[1:] == ([0.5, float(np.float32(0.75 * 2 / 5)), float(np.float32(0.5 / 5))], [3, 1, 0], [6, 2, 1])
    assert one(views, scores, W.AVG, 0.55, views=2)[1:] == ([0.5, 0.25, 0.25], [1, 0, 3], [2, 1, 6])
    assert one(views, scores, W.AVG, 0.55, views=2, max_det=1)[1:] == ([0.5], [1], [2])
    for conf in CONF.values():
        for boxes, scores in ((half, [0.75, 0.25]), (between, [0.75, 0.5, 0.25]), (chain, [0.5, 0.5, 0.25])):
            check_exact(lib, np.array([boxes], np.float64), np.array([scores], np.float32), np.array([len(scores)], np.int32),
                        np.array([0, 1], np.int32), 4, conf, thr=0.3, views=2)


# ------------------------------------------------------------------------------------------------------------------ edges
RANDOM_COUNTS = [63, 64, 65, 255, 256, 257, 1, 0]
IDENTICAL_COUNTS = [300, 1025]
DISJOINT_COUNTS = [LDS_CLUSTERS - 1, LDS_CLUSTERS, LDS_CLUSTERS + 1, 1100]
EDGE_K = 300


@pytest.fixture(scope="module")
def edge_input():
    """One launch: images of 63 ... 257 random candidates, of one candidate and of rows of count 0, an image WITHOUT rows,
    images whose boxes are all identical (one cluster), images whose boxes are all disjoint with equal scores (as many
    clusters as candidates; 319 / 320 / 321 around what LDS holds).  Rows of 300 slots, four to an image."""
    from multibox_amd.synth import merge_candidates
    n_img = len(RANDOM_COUNTS) + len(IDENTICAL_COUNTS) + len(DISJOINT_COUNTS)
    b, s, c, ir = merge_candidates(seed=41, I=n_img, rows_per_image=(4, 4), K=EDGE_K, n_obj=6, count=0)
    s = np.maximum(s, np.float32(1 / 64))
    sizes = RANDOM_COUNTS + IDENTICAL_COUNTS + DISJOINT_COUNTS
    for i, n in enumerate(sizes):
        c[ir[i]:ir[i + 1]] = np.clip(n - EDGE_K * np.arange(4), 0, EDGE_K)
    fb, fs = b.reshape(-1, 4), s.reshape(-1)
    for i in range(len(RANDOM_COUNTS), len(RANDOM_COUNTS) + len(IDENTICAL_COUNTS)):
        fb[ir[i] * EDGE_K:ir[i + 1] * EDGE_K] = [0.125, 0.25, 0.5, 0.75]
    for i in range(len(RANDOM_COUNTS) + len(IDENTICAL_COUNTS), n_img):
        k = np.arange(4 * EDGE_K, dtype=np.float64)
        fb[ir[i] * EDGE_K:ir[i + 1] * EDGE_K] = np.stack([k, 0 * k, k + 0.5, 0 * k + 1], 1)
        fs[ir[i] * EDGE_K:ir[i + 1] * EDGE_K] = 0.5
    ir = np.concatenate([ir[:4], ir[3:]]).astype(np.int32)               # an image without rows after the third
    return b, s, c, ir, sizes[:3] + [0] + sizes[3:]


@pytest.mark.parametrize("conf", sorted(CONF))
def test_stride_edges_in_one_launch(lib, edge_input, conf):
    b, s, c, ir, sizes = edge_input
    max_det = 100
    got, res = check_exact(lib, b, s, c, ir, max_det, CONF[conf], thr=0.55, views=3)
    rc, ob, os_, oi, oc, ost, ov = got
    first_ident, first_disj = 1 + len(RANDOM_COUNTS), 1 + len(RANDOM_COUNTS) + len(IDENTICAL_COUNTS)
    assert oc[3] == 0 and oc[8] == 0 and oc[7] == 1 and ov[7, 0] == 1     # no rows; rows of count 0; one candidate
    for i, n in zip(range(first_ident, first_disj), IDENTICAL_COUNTS):    # one cluster of everybody
        assert oc[i] == 1 and ov[i, 0] == n and oi[i, 0] == int(np.argmax(np.where(np.arange(4 * EDGE_K) < n, s[ir[i]:ir[i + 1]].reshape(-1), -1))) + ir[i] * EDGE_K
    for i, n in zip(range(first_disj, len(ir) - 1), DISJOINT_COUNTS):     # n clusters of one, more than max_det: flat-index order
        assert len(res[i][1]) == n and oc[i] == max_det and (ov[i] == 1).all()
        assert oi[i].tolist() == list(range(ir[i] * EDGE_K, ir[i] * EDGE_K + max_det))


def test_an_image_does_not_depend_on_its_neighbours(lib, edge_input):
    """Every image of the mixed launch gives the bytes of that image launched alone (its flat indices shifted)."""
    b, s, c, ir, sizes = edge_input
    full = run_wbf(lib, b, s, c, ir, 640, W.AVG, views=2)
    assert full[0] == 0
    for i in range(len(ir) - 1):
        a0, a1 = int(ir[i]), int(ir[i + 1])
        if a0 == a1:
            continue
        alone = run_wbf(lib, b[a0:a1], s[a0:a1], c[a0:a1], np.array([0, a1 - a0], np.int32), 640, W.AVG, views=2)
        assert alone[0] == 0
        for j in (1, 2, 4, 5, 6):
            assert alone[j][0].tobytes() == full[j][i].tobytes(), (i, j)
        used = full[3][i] >= 0
        assert np.array_equal(alone[3][0] >= 0, used) and np.array_equal(alone[3][0][used], full[3][i][used] - a0 * EDGE_K)
    assert full[4][-1] == 640                                             # 1 100 disjoint boxes cut to max_det 640


def test_scores_that_take_no_part(lib):
    b = np.zeros((1, 12, 4))
    b[0] = [[0, 0, 10, 10 + 0.25 * k] for k in range(12)]                # all overlap heavily
    above = np.nextafter(np.float32(0.125), np.float32(1))
    s = np.array([[0.25, np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 0.5, 0.125, above, np.nan, 1e-30]], np.float32)
    c, ir = np.array([12], np.int32), np.array([0, 1], np.int32)
    for conf in CONF.values():
        for min_score, members in ((0.0, 5), (0.125, 3), (float(np.float32(1e-30)), 4)):      # at min_score: not live
            got, _ = check_exact(lib, b, s, c, ir, 8, conf, thr=0.5, min_score=min_score)
            assert got[4][0] == 1 and got[3][0, 0] == 7 and got[6][0, 0] == members
    s2 = np.array([[np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0] * 2], np.float32)      # nobody is live
    got, _ = check_exact(lib, b, s2, c, ir, 8, W.AVG)
    assert got[4][0] == 0 and got[5][0] == 0


def test_clamped_counts_k_max_7_and_the_max_det_edges(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=42, I=2, rows_per_image=(3, 3), K=7, n_obj=2)
    s = np.maximum(s, np.float32(1 / 64))
    c = np.array([-3, 100, 7, 0, 2, 9], np.int32)                         # clamped to 0 7 7 | 0 2 7
    for conf in CONF.values():
        clamped = run_wbf(lib, b, s, np.clip(c, 0, 7), ir, 20, conf)
        got = run_wbf(lib, b, s, c, ir, 20, conf)
        assert got[0] == 0 and same_bytes(got, clamped)
        for max_det in (20, 1, 640):
            check_exact(lib, b, s, c, ir, max_det, conf, thr=0.3, views=2)
        got = run_wbf(lib, b, s, c, ir, 641, conf)
        assert got[0] == -2 and all((x == 7).all() for x in got[1:])


@pytest.fixture(scope="module")
def limit_input():
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=12, I=3, rows_per_image=(82, 82), K=200, n_obj=30, count=200)
    c[:82] = 20                                                           # image 0: 1 640 candidates
    c[163] = 185                                                          # image 1: 81 * 200 + 185 = 16 385
    c[245] = 184                                                          # image 2: exactly 16 384
    return b, s, c, ir


def test_candidate_limit_and_max_det_640(lib, limit_input):
    b, s, c, ir = limit_input
    got, res = check_exact(lib, b, s, c, ir, 640, W.AVG, min_score=0.001)
    rc, ob, os_, oi, oc, ost, ov = got
    assert ost.tolist() == [0, 1, 0] and oc[1] == 0 and oc[2] > 0
    assert (oi[1] == -1).all() and not ob[1].any() and not os_[1].any() and not ov[1].any()
    assert oc[2] < int(ov[2].sum()) <= 16384                              # members beyond the founders
    keep = np.r_[0:82, 164:246]                                           # the neighbours are what they are without image 1
    two = run_wbf(lib, b[keep], s[keep], c[keep], np.array([0, 82, 164], np.int32), 640, W.AVG, min_score=0.001)
    for j, full in ((1, ob), (2, os_), (4, oc), (5, ost), (6, ov)):
        assert two[j][0].tobytes() == full[0].tobytes() and two[j][1].tobytes() == full[2].tobytes()


def test_rows_outside_the_input_are_refused_per_image(lib):
    """R is what the workspace was sized for: an image whose rows end past it gets status 2 and touches nothing."""
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=7, I=2, rows_per_image=(2, 2), K=10, n_obj=2, count=10)
    whole = run_wbf(lib, b, s, c, ir, 5, W.AVG)
    got = run_wbf(lib, b, s, c, ir, 5, W.AVG, R=3, ws_bytes=3 * 10 * 88)
    assert got[0] == 0 and got[5].tolist() == [0, 2] and got[4].tolist() == [whole[4][0], 0]
    assert (got[3][1] == -1).all() and not got[1][1].any() and not got[2][1].any() and not got[6][1].any()
    for j in (1, 2, 3, 6):
        assert got[j][0].tobytes() == whole[j][0].tobytes()


def test_unsorted_rows_give_the_same_result(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=8, I=3, rows_per_image=(5, 12), K=40, n_obj=4, count=40)
    rng = np.random.RandomState(0)
    s = ((1 + rng.permutation(s.size)).astype(np.float32) / np.float32(s.size)).reshape(s.shape)      # distinct scores
    srt = np.argsort(-s, axis=1, kind="stable")
    bs, ss = np.take_along_axis(b, srt[:, :, None], 1), np.take_along_axis(s, srt, 1)
    perm = np.stack([rng.permutation(40) for _ in range(len(c))])
    bu, su = np.take_along_axis(bs, perm[:, :, None], 1), np.take_along_axis(ss, perm, 1)
    check_exact(lib, bu, su, c, ir, 30, W.AVG, thr=0.4)
    for conf in CONF.values():
        a, u = run_wbf(lib, bs, ss, c, ir, 30, conf, thr=0.4), run_wbf(lib, bu, su, c, ir, 30, conf, thr=0.4)
        assert a[0] == 0 and u[0] == 0 and same_bytes(a, u, fields=(1, 2, 4, 5, 6))


def test_threshold_one_is_the_plain_top_n(lib, case_inputs):
    """No IoU is > 1: every live candidate founds its own cluster, and with every score live the outputs are
    mbx_merge_detections at +inf, byte for byte."""
    for name in ("topn", "small", "typical"):
        _, max_det, _ = CASES[name]
        b, s, c, ir = case_inputs[name]
        s = s + np.float32(1 / 64)                                        # positive, ties kept
        plain = run_merge(lib, b, s, c, ir, max_det, np.inf)
        for conf in CONF.values():
            wbf = run_wbf(lib, b, s, c, ir, max_det, conf, thr=1.0)
            assert plain[0] == 0 and wbf[0] == 0
            for j in range(1, 6):
                assert wbf[j].tobytes() == plain[j].tobytes(), (name, j)
            assert np.array_equal(wbf[6], (plain[3] >= 0).astype(np.int32))


def test_bad_arguments(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=7, I=2, rows_per_image=(2, 2), K=10, n_obj=2, count=10)
    untouched = lambda got: all((x == 7).all() for x in got[1:])
    nan, inf = float("nan"), float("inf")
    bad = [dict(conf=v) for v in (0, 3, -1)]
    bad += [dict(conf=W.AVG, thr=v) for v in (nan, -0.001, float(np.nextafter(1.0, 2)), inf, -inf)]
    bad += [dict(conf=W.MAX, min_score=v) for v in (nan, -0.001, inf, -inf)]
    bad += [dict(conf=W.AVG, views=v) for v in (0, -1)]
    bad += [dict(conf=W.AVG, ws_bytes=4 * 10 * 88 - 1), dict(conf=W.AVG, ws_bytes=0), dict(conf=W.AVG, R=0), dict(conf=W.AVG, R=-1),
            dict(conf=W.AVG, R=5)]                                        # (five rows need more than the four rows' workspace)
    for kw in bad:
        got = run_wbf(lib, b, s, c, ir, 5, **kw)
        assert got[0] == -1 and untouched(got), kw
    for conf in CONF.values():
        got = run_wbf(lib, b, s, c, ir, 641, conf)
        assert got[0] == -2 and untouched(got)
        got = run_wbf(lib, b, s, c, np.array([0], np.int32), 5, conf)                          # I == 0: nothing launched
        assert got[0] == 0 and untouched(got)
    # the limits of the ranges are accepted
    assert run_wbf(lib, b, s, c, ir, 640, W.AVG, thr=0.0, min_score=0.0, views=1)[0] == 0
    assert run_wbf(lib, b, s, c, ir, 5, W.MAX, thr=1.0, views=2 ** 31 - 1)[0] == 0
    assert lib.mbx_merge_wbf_workspace(0, 10) == 0 and lib.mbx_merge_wbf_workspace(10, 0) == 0 and lib.mbx_merge_wbf_workspace(-1, 10) == 0
    assert lib.mbx_merge_wbf_workspace(2 ** 16, 2 ** 15) == 0 and lib.mbx_merge_wbf_workspace(2 ** 16, 2 ** 15 - 1) == (2 ** 31 - 2 ** 16) * 88
    import torch
    p = torch.zeros(64, dtype=torch.float64, device="cuda").data_ptr()
    call = lambda **kw: lib.mbx_merge_detections_wbf(*[kw.get(k, d) for k, d in (
        ("boxes", p), ("scores", p), ("count", p), ("rows", p), ("R", 1), ("I", 1), ("k_max", 1), ("max_det", 1), ("conf", 1),
        ("thr", 0.55), ("min_score", 0.0), ("views", 1), ("ob", p), ("os", p), ("oi", p), ("oc", p), ("ost", p), ("ov", p), ("ws", p),
        ("ws_bytes", 88), ("stream", None))])
    for name in ("boxes", "scores", "count", "rows", "ob", "os", "oi", "oc", "ost", "ov", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(k_max=0) == -1 and call(max_det=0) == -1 and call(I=-1) == -1 and call(ws_bytes=87) == -1 and call(I=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ ImageMerger
@pytest.mark.parametrize("batch,flush_images", [(4, 1), (64, 1), (4, 256), (64, 3)])
def test_image_merger_wbf_like_one_call(lib, case_inputs, batch, flush_images):
    from multibox_amd.detect import ImageMerger
    _, max_det, thr = CASES["typical"]
    b, s, c, ir = case_inputs["typical"]
    ids = [100 + i for i in range(len(ir) - 1) for _ in range(ir[i + 1] - ir[i])]

    def feed(**kw):
        m = ImageMerger(b.shape[1], max_det, thr, flush_images=flush_images, **kw)
        for a in range(0, len(c), batch):
            m.add(b[a:a + batch], s[a:a + batch], c[a:a + batch], ids[a:a + batch])
        return m.finish()
    for wbf, direct in ((("avg", 0.55, 0.0, 1), dict(conf=W.AVG)), (("max", 0.3, 0.002, 2), dict(conf=W.MAX, thr=0.3, min_score=0.002, views=2))):
        rc, ob, os_, oi, oc, ost, ov = run_wbf(lib, b, s, c, ir, max_det, **direct)
        got_ids, gb, gs, gc = feed(wbf=wbf)
        assert rc == 0 and got_ids == [100 + i for i in range(len(ir) - 1)]
        assert gb.tobytes() == ob.tobytes() and gs.tobytes() == os_.tobytes() and np.array_equal(gc, oc)
    plain = run_merge(lib, b, s, c, ir, max_det, thr)
    got_ids, gb, gs, gc = feed(wbf=None)                                  # off: today's bytes
    assert gb.tobytes() == plain[1].tobytes() and gs.tobytes() == plain[2].tobytes() and np.array_equal(gc, plain[4])
    assert gs.tobytes() != os_.tobytes()
    with pytest.raises(ValueError, match="vote_iou.*soft"):
        ImageMerger(b.shape[1], max_det, thr, wbf=("avg", 0.55, 0.0, 1), vote_iou=0.6)


def test_image_merger_cuts_an_oversize_image_on_the_host_then_fuses(lib, capsys):
    from multibox_amd import records as REC
    from multibox_amd.detect import ImageMerger
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=13, I=3, rows_per_image=(90, 90), K=200, n_obj=12, count=200)
    c[:90], c[180:] = 10, 25                                              # images 0 and 2 small, image 1: 18 000 candidates
    ids = ["a"] * 90 + ["b"] * 90 + ["c"] * 90
    m = ImageMerger(200, 100, None, flush_images=2, wbf=("avg", 0.55, 0.001, 2))
    for a in range(0, len(c), 64):
        m.add(b[a:a + 64], s[a:a + 64], c[a:a + 64], ids[a:a + 64])
    got_ids, gb, gs, gc = m.finish()
    assert got_ids == ["a", "b", "c"] and capsys.readouterr().out.count("WARNING") == 1
    # the oracle on the same cut: image 1's best 16 384 in merge order, as fresh rows
    cut = REC.repack_rows(b[90:180], s[90:180], REC.best_candidates(s[90:180], c[90:180]), 200)
    assert int(cut[2].sum()) == 16384
    for i, (bb, ss, cc) in enumerate(((b[:90], s[:90], c[:90]), cut, (b[180:], s[180:], c[180:]))):
        eb, es, ei, ec, est, ev = W.expected_arrays(W.wbf_oracle(bb, ss, cc, np.array([0, len(cc)]), W.AVG, 0.55, 0.001, 2), 100)
        assert gc[i] == ec[0] and gb[i].tobytes() == eb[0].tobytes() and gs[i].tobytes() == es[0].tobytes(), i


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_wbf_key(cli_setup):
    """detect.py --merge_per_image with DETECTION.MERGE_WBF avg (expected views 2), and null: the merged file is the oracle
    applied to the dense output, the run without the key is unchanged."""
    d = cli_setup
    (d / "config_wbf.yaml").write_text(CFG + "  MERGE_WBF : avg\n  MERGE_WBF_EXPECTED_VIEWS : 2\n  MERGE_WBF_IOU_THRESHOLD : 0.5\n")
    (d / "config_wbf_null.yaml").write_text(CFG + "  MERGE_WBF : null\n")
    _run(_detect_cmd(d, "merged", "--merge_per_image", "--max_detections", "20"))
    for cfg, out in (("config_wbf.yaml", "wbf"), ("config_wbf_null.yaml", "wbf_null")):
        cmd = _detect_cmd(d, out, "--merge_per_image", "--max_detections", "20")
        cmd[cmd.index("--config") + 1] = str(d / cfg)
        _run(cmd)
    read = lambda out, name: open(d / out / name, "rb").read()
    assert read("wbf", "results-dense-0.json") == read("merged", "results-dense-0.json")
    assert read("wbf_null", "results-merged-0.json") == read("merged", "results-merged-0.json")
    groups = []                                                           # consecutive image_id = one image
    for x in json.loads(read("wbf", "results-dense-0.json")):
        if not groups or groups[-1][0] != x["image_id"]:
            groups.append((x["image_id"], []))
        groups[-1][1].append(x)
    assert [gid for gid, _ in groups] == [1000, 1001, 1002]
    want = []
    for gid, xs in groups:
        s = np.array([x["score"] for x in xs], np.float32)
        assert [float(v) for v in s] == [x["score"] for x in xs]           # JSON round-trips the float32 scores exactly
        F, sc, first, n = W.wbf(np.array([x["bbox"] for x in xs], np.float64), s, W.AVG, 0.5, 0.0, 2)
        assert len(xs) > 20 and len(sc) > 0
        want += [{"image_id": gid, "bbox": F[k].tolist(), "score": float(sc[k])} for k in range(min(len(sc), 20))]
    got = json.loads(read("wbf", "results-merged-0.json"))
    print("dense records", [len(xs) for _, xs in groups], "fused records", len(got))
    assert got == want and got != json.loads(read("merged", "results-merged-0.json"))
