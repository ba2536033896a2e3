"""mbx_merge_detections_voted (the per-image merge with box voting), ImageMerger(vote_iou=) and detect.py's
DETECTION.MERGE_VOTE_IOU_THRESHOLD, on the GPU.  The kept list is compared bit for bit with a plain mbx_merge_detections
call in the same test; voters and voted boxes come from tests/vote_oracle.py (numpy + fractions), the boxes within the
derived bound  |got - exact| <= (2 n + 4) * 2^-53 * sum(w |x|) / sum(w)  per coordinate, n = the number of voters."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.merge_oracle import CASES
from tests.test_gpu_merge import CFG, _detect_cmd, _run, cli_setup, lib, run_merge  # noqa: F401  (fixtures and helpers)
from tests.vote_oracle import bound, image_candidates, vote_exact

pytestmark = pytest.mark.gpu


def run_voted(lib, boxes, scores, count, image_rows, max_det, thr, vthr, votes=True):
    """One call; (rc, out_boxes, out_scores, out_src, out_count, out_status, out_votes) as numpy, pre-filled with 7."""
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
    rc = lib.mbx_merge_detections_voted(d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), I, K, max_det, float(thr),
                                        float(vthr), o_b.data_ptr(), o_s.data_ptr(), o_i.data_ptr(), o_c.data_ptr(),
                                        o_st.data_ptr(), o_v.data_ptr() if votes else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (o_b, o_s, o_i, o_c, o_st, o_v))


def check_voted(lib, boxes, scores, count, image_rows, max_det, thr, vthr, images=None):
    """The voted call against the plain call (kept list, bit for bit) and the oracle (votes, boxes within the bound); a
    second call gives the same bytes.  Returns the voted call's outputs and the votes of the used slots."""
    plain = run_merge(lib, boxes, scores, count, image_rows, max_det, thr)
    got = run_voted(lib, boxes, scores, count, image_rows, max_det, thr, vthr)
    again = run_voted(lib, boxes, scores, count, image_rows, max_det, thr, vthr)
    assert plain[0] == 0 and got[0] == 0 and again[0] == 0
    for a, b in zip(got[1:], again[1:]):
        assert a.tobytes() == b.tobytes()
    rc, ob, os_, oi, oc, ost, ov = got
    assert os_.tobytes() == plain[2].tobytes() and np.array_equal(oi, plain[3])
    assert np.array_equal(oc, plain[4]) and np.array_equal(ost, plain[5])
    fb, fs = boxes.reshape(-1, 4), scores.reshape(-1)
    all_votes, worst = [], Fraction(0)
    for i in (range(len(image_rows) - 1) if images is None else images):
        nk = int(oc[i])
        assert not ov[i, nk:].any() and not ob[i, nk:].any()              # unused slots
        src = oi[i, :nk].astype(np.int64)
        cand = image_candidates(scores, count, int(image_rows[i]), int(image_rows[i + 1])) if ost[i] == 0 else np.zeros(0, np.int64)
        mean, absmean, n = vote_exact(fb[src], fb[cand], fs[cand], vthr)
        assert np.array_equal(ov[i, :nk], n), (i, ov[i, :nk].tolist(), n.tolist())
        for k in range(nk):
            if n[k] == 0:
                assert ob[i, k].tobytes() == fb[src[k]].tobytes(), (i, k)
                continue
            for j in range(4):
                err, lim = abs(Fraction(float(ob[i, k, j])) - mean[k][j]), bound(n[k], absmean[k][j])
                assert err <= lim, (i, k, j, float(err), float(lim))
                if lim > 0:
                    worst = max(worst, err / lim)
        all_votes.append(n)
    v = np.concatenate(all_votes + [np.zeros(0, np.int64)])
    print("vote iou %.2f: kept %s  votes min %d median %d max %d, %d without voters  worst error / bound %.3g"
          % (vthr, oc.tolist(), v.min() if len(v) else 0, np.median(v) if len(v) else 0, v.max() if len(v) else 0,
             int((v == 0).sum()), float(worst)))
    return got, v


@pytest.fixture(scope="module")
def case_inputs():
    from multibox_amd.synth import merge_candidates
    return {name: merge_candidates(**kw) for name, (kw, _, _) in CASES.items()}


@pytest.mark.parametrize("vthr", [0.6, 0.9])
@pytest.mark.parametrize("name", sorted(CASES))
def test_generator_cases(lib, case_inputs, name, vthr):
    """The five seeded cases of the plain merge (`topn` has iou_threshold = +inf: plain top-N, with voting)."""
    _, max_det, thr = CASES[name]
    b, s, c, ir = case_inputs[name]
    got, v = check_voted(lib, b, s, c, ir, max_det, thr, vthr)
    if name == "small":
        assert (v == 0).any()                                             # kept boxes without a voter (degenerate ones): own bytes
    if name == "clusters" and vthr == 0.6:
        assert np.median(v) == 133 and v.max() == 682                     # many passes of a wavefront over the candidates
    # voting moved boxes: it is not the plain result
    assert got[1].tobytes() != run_merge(lib, b, s, c, ir, max_det, thr)[1].tobytes()


def test_known_answers_bit_exact(lib):
    one, rows = np.array([2], np.int32), np.array([0, 1], np.int32)
    b = np.array([[[0, 0, 10, 10], [0, 0, 10, 12]]], np.float64)
    s = np.array([[0.75, 0.25]], np.float32)
    rc, ob, os_, oi, oc, ost, ov = run_voted(lib, b, s, one, rows, 4, 0.5, 0.5)
    assert rc == 0 and oc[0] == 1 and oi[0].tolist() == [0, -1, -1, -1] and ov[0].tolist() == [2, 0, 0, 0]
    assert ob[0].tobytes() == np.array([[0, 0, 10, 10.5], [0] * 4, [0] * 4, [0] * 4], np.float64).tobytes()
    # >=: an IoU of exactly 0.5 votes at 0.5 and not one ulp above (nothing is suppressed: 0.5 is not > 0.5)
    b = np.array([[[0, 0, 2, 2], [0, 0, 2, 4]]], np.float64)
    rc, ob, os_, oi, oc, ost, ov = run_voted(lib, b, s, one, rows, 2, 0.5, 0.5)
    assert rc == 0 and oc[0] == 2 and ov[0].tolist() == [2, 2]
    assert ob[0].tobytes() == np.array([[0, 0, 2, 2.5], [0, 0, 2, 2.5]], np.float64).tobytes()
    rc, ob, os_, oi, oc, ost, ov = run_voted(lib, b, s, one, rows, 2, 0.5, np.nextafter(0.5, 1))
    assert rc == 0 and oc[0] == 2 and ov[0].tolist() == [1, 1] and ob[0].tobytes() == b[0].tobytes()
    # a vote threshold of 1: duplicates only
    rc, ob, os_, oi, oc, ost, ov = run_voted(lib, b, s, one, rows, 2, 0.5, 1.0)
    assert rc == 0 and ov[0].tolist() == [1, 1] and ob[0].tobytes() == b[0].tobytes()


def test_who_does_not_vote(lib):
    rows = np.array([0, 1], np.int32)
    # scores 0, -0, -1, NaN, +inf: kept (top-N, no suppression) but no voters for anyone; all seven overlap at IoU >= 10/12
    b = np.array([[[0, 0, 10, 10 + 0.25 * k] for k in range(7)]], np.float64)
    s = np.array([[0.5, 0.0, -0.0, -1.0, np.nan, np.inf, 0.25]], np.float32)
    (rc, ob, os_, oi, oc, ost, ov), v = check_voted(lib, b, s, np.array([7], np.int32), rows, 8, np.inf, 0.6)
    assert oc[0] == 7 and oi[0, :7].tolist() == [4, 5, 0, 6, 1, 2, 3] and ov[0].tolist() == [2] * 7 + [0]
    want = (0.5 * 10.0 + 0.25 * 11.5) / 0.75                            # slots 0 and 6; dyadic, so nothing is rounded but the division
    assert (ob[0, :7, :3] == [0, 0, 10]).all() and np.abs(ob[0, :7, 3] - want).max() <= 2 ** -49
    # a slot at or past count[r] holding a large-score duplicate of the kept box changes nothing
    b2 = np.array([[[0, 0, 10, 10], [0, 0, 10, 12], [0, 0, 10, 10], [0, 0, 10, 10]]], np.float64)
    s2 = np.array([[0.75, 0.25, 1000.0, 1000.0]], np.float32)
    b0, s0 = b2.copy(), s2.copy()
    b0[0, 2:], s0[0, 2:] = 0, 0
    g2, g0 = (run_voted(lib, bb, ss, np.array([2], np.int32), rows, 3, 0.5, 0.5) for bb, ss in ((b2, s2), (b0, s0)))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(g2[1:], g0[1:]))
    assert g2[6][0].tolist() == [2, 0, 0] and g2[1][0, 0].tolist() == [0, 0, 10, 10.5]
    # a candidate past the max_det cut votes (nothing suppressed at threshold 1; max_det = 1 keeps the first only)
    rc, ob, os_, oi, oc, ost, ov = run_voted(lib, b2, s2, np.array([2], np.int32), rows, 1, 1.0, 0.5)
    assert rc == 0 and oc[0] == 1 and ov[0].tolist() == [2] and ob[0, 0].tolist() == [0, 0, 10, 10.5] and os_[0, 0] == 0.75
    # a kept box of zero area: no voters (not even its duplicate), its own bytes
    b3 = np.array([[[1, 1, 1, 3], [1, 1, 1, 3], [0, 0, 4, 4]]], np.float64)
    s3 = np.array([[0.9, 0.8, 0.7]], np.float32)
    (rc, ob, os_, oi, oc, ost, ov), v = check_voted(lib, b3, s3, np.array([3], np.int32), rows, 4, 0.5, 0.6)
    assert oc[0] == 3 and ov[0].tolist() == [0, 0, 1, 0] and ob[0, :3].tobytes() == b3[0].tobytes()


def test_an_image_does_not_depend_on_its_neighbours(lib, case_inputs):
    """Image 3 of `typical` alone, among the eight, and with the eight in reverse order: the same bytes."""
    _, max_det, thr = CASES["typical"]
    b, s, c, ir = case_inputs["typical"]
    K, I = s.shape[1], len(ir) - 1
    full = run_voted(lib, b, s, c, ir, max_det, thr, 0.6)
    a0, a1 = int(ir[3]), int(ir[4])
    alone = run_voted(lib, b[a0:a1], s[a0:a1], c[a0:a1], np.array([0, a1 - a0], np.int32), max_det, thr, 0.6)
    order = list(range(I))[::-1]
    sel = np.concatenate([np.arange(ir[i], ir[i + 1]) for i in order])
    rrows = np.concatenate([[0], np.cumsum([ir[i + 1] - ir[i] for i in order])]).astype(np.int32)
    rev = run_voted(lib, b[sel], s[sel], c[sel], rrows, max_det, thr, 0.6)
    assert full[0] == 0 and alone[0] == 0 and rev[0] == 0 and full[4][3] == max_det
    for got, at, row0 in ((alone, 0, 0), (rev, order.index(3), int(rrows[order.index(3)]))):
        for j in (1, 2, 4, 5, 6):                                         # boxes, scores, count, status, votes
            assert got[j][at].tobytes() == full[j][3].tobytes(), j
        assert np.array_equal(got[3][at] - row0 * K, full[3][3] - a0 * K)                   # flat indices, from the image's first row
    assert full[6][3].max() > 1


def test_candidate_limit_and_max_det_640(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=12, I=3, rows_per_image=(82, 82), K=200, n_obj=30, count=200)
    c[:82] = 20                                                           # image 0: 1 640 candidates
    c[163] = 185                                                          # image 1: 81 * 200 + 185 = 16 385
    c[245] = 184                                                          # image 2: exactly 16 384
    (rc, ob, os_, oi, oc, ost, ov), v = check_voted(lib, b, s, c, ir, 640, 0.5, 0.6)
    assert ost.tolist() == [0, 1, 0]
    assert oc[1] == 0 and not ov[1].any() and not ob[1].any() and (oi[1] == -1).all() and not os_[1].any()
    assert oc[2] > 512 and ov[2].max() > 64                               # more kept boxes than 512, and voters beyond one pass of a wavefront
    # the neighbours are what they are without image 1
    keep = np.r_[0:82, 164:246]
    two = run_voted(lib, b[keep], s[keep], c[keep], np.array([0, 82, 164], np.int32), 640, 0.5, 0.6)
    for j in (1, 2, 4, 5, 6):
        assert two[j][0].tobytes() == (ob, os_, oi, oc, ost, ov)[j - 1][0].tobytes() and two[j][1].tobytes() == (ob, os_, oi, oc, ost, ov)[j - 1][2].tobytes()


def test_empty_inputs(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=7, I=2, rows_per_image=(2, 2), K=10, n_obj=2, count=10)
    got = run_voted(lib, b, s, c, np.array([0], np.int32), 5, 0.5, 0.6)                       # I = 0: nothing launched
    assert got[0] == 0 and all((x == 7).all() for x in got[1:])
    # an image whose rows all have count 0, beside one that has candidates; an image without rows
    (rc, ob, os_, oi, oc, ost, ov), v = check_voted(lib, b, s, np.array([0, -3, 10, 10], np.int32), ir, 5, 0.5, 0.6)
    assert oc[0] == 0 and ost[0] == 0 and not ov[0].any() and not ob[0].any() and (oi[0] == -1).all() and oc[1] > 0
    check_voted(lib, b, s, c, np.array([0, 2, 2, 4], np.int32), 5, 0.5, 0.6)
    # top-N (iou_threshold = +inf) with voting
    check_voted(lib, b, s, c, ir, 7, np.inf, 0.6)


def test_bad_arguments(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=7, I=2, rows_per_image=(2, 2), K=10, n_obj=2, count=10)
    untouched = lambda got: all((x == 7).all() for x in got[1:])
    for vthr in (0.0, -0.0, -0.1, 1.5, np.nextafter(1.0, 2), np.nan, np.inf, -np.inf):
        got = run_voted(lib, b, s, c, ir, 5, 0.5, vthr)
        assert got[0] == -1 and untouched(got), vthr
    got = run_voted(lib, b, s, c, ir, 5, 0.5, 0.6, votes=False)                                  # null out_votes
    assert got[0] == -1 and untouched(got)
    got = run_voted(lib, b, s, c, ir, 641, 0.5, 0.6)
    assert got[0] == -2 and untouched(got)
    assert run_voted(lib, b, s, c, ir, 640, 0.5, 1.0)[0] == 0 and run_voted(lib, b, s, c, ir, 5, 0.5, 5e-324)[0] == 0
    import torch
    p = torch.zeros(64, dtype=torch.float64, device="cuda").data_ptr()
    call = lambda **kw: lib.mbx_merge_detections_voted(*[kw.get(k, d) for k, d in (
        ("boxes", p), ("scores", p), ("count", p), ("rows", p), ("I", 1), ("k_max", 1), ("max_det", 1), ("thr", 0.5), ("vthr", 0.5),
        ("ob", p), ("os", p), ("oi", p), ("oc", p), ("ost", p), ("ov", p), ("stream", None))])
    for name in ("boxes", "scores", "count", "rows", "ob", "os", "oi", "oc", "ost", "ov"):
        assert call(**{name: None}) == -1, name
    assert call(k_max=0) == -1 and call(max_det=0) == -1 and call(I=-1) == -1 and call(I=0) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("batch,flush_images", [(4, 1), (64, 1), (4, 256), (64, 256)])
def test_image_merger_votes_like_one_call(lib, case_inputs, batch, flush_images):
    from multibox_amd.detect import ImageMerger
    _, max_det, thr = CASES["typical"]
    b, s, c, ir = case_inputs["typical"]
    ids = [100 + i for i in range(len(ir) - 1) for _ in range(ir[i + 1] - ir[i])]

    def feed(**kw):
        m = ImageMerger(b.shape[1], max_det, thr, flush_images=flush_images, **kw)
        for a in range(0, len(c), batch):
            m.add(b[a:a + batch], s[a:a + batch], c[a:a + batch], ids[a:a + batch])
        return m.finish()
    rc, ob, os_, oi, oc, ost, ov = run_voted(lib, b, s, c, ir, max_det, thr, 0.6)
    got_ids, gb, gs, gc = feed(vote_iou=0.6)
    assert rc == 0 and got_ids == [100 + i for i in range(len(ir) - 1)]
    assert gb.tobytes() == ob.tobytes() and gs.tobytes() == os_.tobytes() and np.array_equal(gc, oc)
    plain = run_merge(lib, b, s, c, ir, max_det, thr)
    for kw in ({}, {"vote_iou": None}):                                   # off: today's plain result
        got_ids, gb, gs, gc = feed(**kw)
        assert gb.tobytes() == plain[1].tobytes() and gs.tobytes() == plain[2].tobytes() and np.array_equal(gc, plain[4])
    assert ob.tobytes() != plain[1].tobytes()
    with pytest.raises(ValueError):
        ImageMerger(b.shape[1], max_det, thr, vote_iou=1.5)


def test_cli_vote_key(cli_setup):
    """detect.py --merge_per_image with and without DETECTION.MERGE_VOTE_IOU_THRESHOLD: the same detections in the same
    order with the same scores, boxes moved; the dense file does not change."""
    d = cli_setup
    (d / "config_vote.yaml").write_text(CFG + "  MERGE_VOTE_IOU_THRESHOLD : 0.5\n")
    _run(_detect_cmd(d, "merged", "--merge_per_image", "--max_detections", "20"))
    cmd = _detect_cmd(d, "voted", "--merge_per_image", "--max_detections", "20")
    cmd[cmd.index("--config") + 1] = str(d / "config_vote.yaml")
    _run(cmd)
    assert open(d / "voted" / "results-dense-0.json", "rb").read() == open(d / "merged" / "results-dense-0.json", "rb").read()
    plain, voted = (json.load(open(d / n / "results-merged-0.json")) for n in ("merged", "voted"))
    assert len(plain) == len(voted) > 3
    assert [(x["image_id"], x["score"]) for x in plain] == [(x["image_id"], x["score"]) for x in voted]
    moved = sum(x["bbox"] != y["bbox"] for x, y in zip(plain, voted))
    shift = max(abs(u - v) for x, y in zip(plain, voted) for u, v in zip(x["bbox"], y["bbox"]))
    print("merged records", len(plain), "moved by voting", moved, "largest coordinate shift %.4g" % shift)
    assert moved >= 1
