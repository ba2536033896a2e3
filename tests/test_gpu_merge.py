"""mbx_merge_detections (per-image merge of multi-crop detections: score order, greedy NMS across patches, top-N), the
host class that feeds it (multibox_amd.detect.ImageMerger) and detect.py --merge_per_image, on the GPU.  Every expected
value comes from tests/merge_oracle.py (oracle.ref_numpy.nms_greedy + numpy) or is hand-made."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.merge_oracle import CASES, expected_arrays, merge_oracle, nms_first

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


def run_merge(lib, boxes, scores, count, image_rows, max_det, thr):
    """One launch; (rc, out_boxes, out_scores, out_src, out_count, out_status) as numpy."""
    import torch
    boxes, scores = np.ascontiguousarray(boxes, np.float64), np.ascontiguousarray(scores, np.float32)
    R, K = scores.shape
    assert boxes.shape == (R, K, 4) and len(count) == R and int(image_rows[-1]) <= R
    I = len(image_rows) - 1
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).cuda() if np.size(a) else torch.zeros(1, dtype=getattr(torch, np.dtype(dt).name)).cuda()
    d_b, d_s, d_c, d_r = dev(boxes, np.float64), dev(scores, np.float32), dev(count, np.int32), dev(image_rows, np.int32)
    n = max(I, 1)
    o_b = torch.full((n, max_det, 4), 7.0, dtype=torch.float64, device="cuda")
    o_s = torch.full((n, max_det), 7.0, dtype=torch.float32, device="cuda")
    o_i = torch.full((n, max_det), 7, dtype=torch.int32, device="cuda")
    o_c = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    o_st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    rc = lib.mbx_merge_detections(d_b.data_ptr(), d_s.data_ptr(), d_c.data_ptr(), d_r.data_ptr(), I, K, max_det, float(thr),
                                  o_b.data_ptr(), o_s.data_ptr(), o_i.data_ptr(), o_c.data_ptr(), o_st.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (o_b, o_s, o_i, o_c, o_st))


def check_against_oracle(lib, boxes, scores, count, image_rows, max_det, thr):
    kept = merge_oracle(boxes, scores, count, image_rows, max_det, thr)
    eb, es, ei, ec = expected_arrays(boxes, scores, kept, max_det)
    rc, ob, os_, oi, oc, ost = run_merge(lib, boxes, scores, count, image_rows, max_det, thr)
    assert rc == 0
    print("candidates", [int(np.clip(count[image_rows[i]:image_rows[i + 1]], 0, scores.shape[1]).sum()) for i in range(len(kept))],
          "kept", ec.tolist(), "device", oc.tolist())
    assert not ost.any()
    assert np.array_equal(oc, ec)
    assert np.array_equal(oi, ei)
    assert os_.tobytes() == es.tobytes()
    assert ob.tobytes() == eb.tobytes()                                  # kept boxes: the source's bytes; unused slots 0
    return kept


@pytest.mark.parametrize("name", sorted(CASES))
def test_generator_cases(lib, name):
    """The five seeded cases: both exits of the walk (max_det reached: typical / wide / topn; list exhausted: small / clusters,
    the latter with >= 4 000 candidates per image), ties in every image, rows with count 0."""
    from multibox_amd.synth import merge_candidates
    kw, max_det, thr = CASES[name]
    b, s, c, ir = merge_candidates(**kw)
    kept = check_against_oracle(lib, b, s, c, ir, max_det, thr)
    n = [len(k) for k in kept]
    if name in ("typical", "wide", "topn"):
        assert min(n) == max_det
    else:
        assert max(n) < max_det
    if name == "clusters":
        assert min(int(c[ir[i]:ir[i + 1]].sum()) for i in range(len(ir) - 1)) >= 4000


def test_empty_inputs(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=7, I=2, rows_per_image=(2, 2), K=10, n_obj=2, count=10)
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, c, np.array([0], np.int32), 5, 0.5)         # I = 0: nothing launched
    assert rc == 0 and (oc == 7).all() and (oi == 7).all()
    # an image without rows between two others
    ir3 = np.array([0, 2, 2, 4], np.int32)
    check_against_oracle(lib, b, s, c, ir3, 5, 0.5)
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, c, ir3, 5, 0.5)
    assert oc[1] == 0 and ost[1] == 0 and (oi[1] == -1).all() and not ob[1].any() and not os_[1].any()
    # all counts 0; counts outside [0, k_max] are clamped
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, np.array([0, -3, 0, 0], np.int32), ir, 5, 0.5)
    assert rc == 0 and not oc.any() and not ost.any() and (oi == -1).all() and not ob.any()
    big = np.array([10, 1000, 10, 10], np.int32)
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, big, ir, 5, 0.5)
    eb, es, ei, ec = expected_arrays(b, s, merge_oracle(b, s, c, ir, 5, 0.5), 5)
    assert rc == 0 and np.array_equal(oi, ei) and np.array_equal(oc, ec)
    # one candidate
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, np.array([0, 0, 1, 0], np.int32), ir, 5, 0.5)
    assert oc.tolist() == [0, 1] and oi[1].tolist() == [20, -1, -1, -1, -1] and ob[1, 0].tobytes() == b[2, 0].tobytes()
    assert os_[1, 0] == s[2, 0]


def test_unsorted_rows_give_the_same_result(lib):
    """The kernel does not assume that a row is sorted: the same candidates with the slots of every row shuffled."""
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=8, I=3, rows_per_image=(5, 12), K=40, n_obj=4, count=40)
    rng = np.random.RandomState(0)
    s = (rng.permutation(s.size).astype(np.float32) / np.float32(s.size)).reshape(s.shape)      # distinct scores: no tie to break
    srt = np.argsort(-s, axis=1, kind="stable")
    bs, ss = np.take_along_axis(b, srt[:, :, None], 1), np.take_along_axis(s, srt, 1)
    perm = np.stack([rng.permutation(40) for _ in range(len(c))])
    bu, su = np.take_along_axis(bs, perm[:, :, None], 1), np.take_along_axis(ss, perm, 1)
    check_against_oracle(lib, bs, ss, c, ir, 30, 0.4)
    check_against_oracle(lib, bu, su, c, ir, 30, 0.4)
    a, u = run_merge(lib, bs, ss, c, ir, 30, 0.4), run_merge(lib, bu, su, c, ir, 30, 0.4)
    assert a[1].tobytes() == u[1].tobytes() and a[2].tobytes() == u[2].tobytes() and np.array_equal(a[4], u[4])


def test_no_threshold_is_plain_top_n(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=9, I=2, rows_per_image=(20, 30), K=30, n_obj=2, unrelated=0.0)
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, c, ir, 64, np.inf)
    assert rc == 0
    for i in range(2):
        flat = np.concatenate([np.arange(r * 30, r * 30 + c[r]) for r in range(ir[i], ir[i + 1])])
        top = flat[np.argsort(-s.reshape(-1)[flat], kind="stable")][:64]
        assert oc[i] == 64 and np.array_equal(oi[i], top)
        assert ob[i].tobytes() == b.reshape(-1, 4)[top].tobytes()         # heavy overlap, nothing suppressed
    assert run_merge(lib, b, s, c, ir, 64, 0.5)[4].max() < 64              # with a threshold the same input is thinned


def test_known_answers_and_the_strict_rule(lib):
    """The hand-made five boxes of tests/test_host_logic.py::test_oracle_nms_known_answers, spread over two rows."""
    b = np.zeros((2, 3, 4))
    b.reshape(-1, 4)[:5] = [[0, 0, 1, 1], [0, 0, 1, .5], [.5, .5, 1.5, 1.5], [2, 2, 3, 3], [0, 0, 1, 1]]
    s = np.array([[.9, .8, .7], [.6, .5, 0]], np.float32)
    c, ir = np.array([3, 2], np.int32), np.array([0, 2], np.int32)
    # flat indices: row 0 -> 0 1 2, row 1 -> 3 4.  IoU(0,1) = .5, IoU(0,2) = .25/1.75, IoU(0,4) = 1, IoU(1,2) = 0
    for thr, want in ((0.5, [0, 1, 2, 3]), (0.49, [0, 2, 3]), (0.1, [0, 3]), (1.0, [0, 1, 2, 3, 4])):
        rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, c, ir, 8, thr)
        assert rc == 0 and oc[0] == len(want) and oi[0, :len(want)].tolist() == want and (oi[0, len(want):] == -1).all(), thr
    # max_det stops the walk
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, c, ir, 2, 1.0)
    assert oc[0] == 2 and oi[0].tolist() == [0, 1]
    # equal scores: ascending flat index; the exact duplicate (4) of box 0 goes, at 1.0 it stays
    s2 = np.full((2, 3), .5, np.float32)
    assert run_merge(lib, b, s2, c, ir, 8, 0.99)[3][0, :4].tolist() == [0, 1, 2, 3]
    assert run_merge(lib, b, s2, c, ir, 8, 1.0)[3][0, :5].tolist() == [0, 1, 2, 3, 4]


def test_nan_sorts_first_and_zeros_tie(lib):
    b = np.zeros((1, 4, 4))
    b[0] = [[0, 0, .1, .1], [.2, .2, .3, .3], [.4, .4, .5, .5], [.6, .6, .7, .7]]          # disjoint
    s = np.array([[0.0, np.nan, -0.0, 0.5]], np.float32)
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, np.array([4], np.int32), np.array([0, 1], np.int32), 4, 0.5)
    assert rc == 0 and oc[0] == 4 and oi[0].tolist() == [1, 3, 0, 2]                          # NaN, 0.5, then +0 / -0 by index
    assert np.isnan(os_[0, 0]) and os_[0, 1:].tobytes() == np.array([0.5, 0.0, -0.0], np.float32).tobytes()


def test_candidate_limit_and_max_det_512(lib):
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=12, I=3, rows_per_image=(82, 82), K=200, n_obj=30, count=200)
    c[:82] = 20                                                           # image 0: 1 640 candidates
    c[82:164] = 200
    c[163] = 185                                                          # image 1: 81 * 200 + 185 = 16 385
    c[164:] = 200
    c[245] = 184                                                          # image 2: exactly 16 384
    kept = merge_oracle(b, s, c, ir, 512, 0.5)
    eb, es, ei, ec = expected_arrays(b, s, kept, 512)
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, c, ir, 512, 0.5)
    print("kept", ec.tolist(), "device", oc.tolist(), "status", ost.tolist())
    assert rc == 0 and ost.tolist() == [0, 1, 0]
    assert oc[1] == 0 and (oi[1] == -1).all() and not ob[1].any() and not os_[1].any()
    for i in (0, 2):                                                      # its neighbours in the same launch
        assert oc[i] == ec[i] and np.array_equal(oi[i], ei[i]) and ob[i].tobytes() == eb[i].tobytes() and os_[i].tobytes() == es[i].tobytes()
    assert ec[2] == 512                                                   # max_det 512 beside the full 16 384 keys


def test_bad_arguments(lib):
    import torch
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    call = lambda **kw: lib.mbx_merge_detections(*[kw.get(k, d) for k, d in (
        ("boxes", p), ("scores", p), ("count", p), ("rows", p), ("I", 1), ("k_max", 1), ("max_det", 1), ("thr", 0.5),
        ("ob", p), ("os", p), ("oi", p), ("oc", p), ("ost", p), ("stream", None))])
    for name in ("boxes", "scores", "count", "rows", "ob", "os", "oi", "oc", "ost"):
        assert call(**{name: None}) == -1, name
    assert call(k_max=0) == -1 and call(max_det=0) == -1 and call(max_det=-5) == -1 and call(I=-1) == -1
    assert call(max_det=100000) == -2
    assert call(I=0) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def stream_case():
    """320-odd rows of eight images (the `typical` case) with their ids and the oracle's answer."""
    from multibox_amd.synth import merge_candidates
    kw, max_det, thr = CASES["typical"]
    b, s, c, ir = merge_candidates(**kw)
    ids = [100 + i for i in range(len(ir) - 1) for _ in range(ir[i + 1] - ir[i])]
    return b, s, c, ir, ids, expected_arrays(b, s, merge_oracle(b, s, c, ir, max_det, thr), max_det), max_det, thr


@pytest.mark.parametrize("flush_images", [1, 3, 256])
@pytest.mark.parametrize("batch", [4, 64, 256])
def test_image_merger_batches_straddle_images(lib, stream_case, batch, flush_images):
    from multibox_amd.detect import ImageMerger
    b, s, c, ir, ids, (eb, es, ei, ec), max_det, thr = stream_case
    m = ImageMerger(b.shape[1], max_det, thr, flush_images=flush_images)
    for a in range(0, len(c), batch):
        bb, sb, cb = b[a:a + batch].copy(), s[a:a + batch].copy(), c[a:a + batch].copy()
        m.add(bb, sb, cb, ids[a:a + batch])
        bb[:], sb[:], cb[:] = -1, -1, 0                                   # the caller reuses its buffers: add() must have copied
    got_ids, gb, gs, gc = m.finish()
    assert got_ids == [100 + i for i in range(len(ir) - 1)]
    assert np.array_equal(gc, ec) and gb.tobytes() == eb.tobytes() and gs.tobytes() == es.tobytes()
    # equal to one launch over everything
    rc, ob, os_, oi, oc, ost = run_merge(lib, b, s, c, ir, max_det, thr)
    assert rc == 0 and ob.tobytes() == gb.tobytes() and os_.tobytes() == gs.tobytes() and np.array_equal(oc, gc)
    assert m.finish()[0] == []                                            # nothing left


def test_image_merger_cuts_an_oversize_image_on_the_host(lib, capsys):
    from multibox_amd.detect import ImageMerger
    from multibox_amd.synth import merge_candidates
    b, s, c, ir = merge_candidates(seed=13, I=3, rows_per_image=(90, 90), K=200, n_obj=12, count=200)
    c[:90], c[180:] = 10, 25                                              # images 0 and 2 small, image 1: 18 000 candidates
    ids = ["a"] * 90 + ["b"] * 90 + ["c"] * 90
    eb, es, ei, ec = expected_arrays(b, s, merge_oracle(b, s, c, ir, 100, 0.5), 100)       # the oracle cuts at 16 384 too
    m = ImageMerger(200, 100, 0.5, flush_images=2)
    for a in range(0, len(c), 64):
        m.add(b[a:a + 64], s[a:a + 64], c[a:a + 64], ids[a:a + 64])
    got_ids, gb, gs, gc = m.finish()
    assert got_ids == ["a", "b", "c"] and np.array_equal(gc, ec) and gb.tobytes() == eb.tobytes() and gs.tobytes() == es.tobytes()
    assert capsys.readouterr().out.count("WARNING") == 1


# ------------------------------------------------------------------------------------------------------------------ CLI
CFG = """
NUM_BBOXES_PER_CELL : 5
MAX_NUM_BBOXES : 13
LOCATION_LOSS_ALPHA : 1000.0
BATCH_SIZE : 4
INPUT_SIZE : 299
NUM_TRAIN_EXAMPLES : 56945
NUM_TRAIN_ITERATIONS : 1000000
DETECTION :
  USE_ORIGINAL_IMAGE : true
  ORIGINAL_IMAGE_MAX_TO_KEEP : 200
  USE_FLIPPED_ORIGINAL_IMAGE : true
  FLIPPED_IMAGE_MAX_TO_KEEP : 100
  CROPS :
    - HEIGHT : 299
      WIDTH : 299
      HEIGHT_STRIDE : 113
      WIDTH_STRIDE : 113
      FLIP : false
      MAX_TO_KEEP : 50
"""


@pytest.fixture(scope="module")
def cli_setup(tmp_path_factory):
    """Three JPEG images = 12 patches, BATCH_SIZE 4 (batches cut through images), an untrained checkpoint."""
    import __graft_entry__ as g
    g.build()
    import torch
    from multibox_amd import priors as PR, checkpoint as CK
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer
    from tests.test_inputs_cpu import _make_records
    d = tmp_path_factory.mktemp("merge_cli")
    (d / "config.yaml").write_text(CFG)
    priors = PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.])
    PR.save_priors(str(d / "priors.pkl"), priors)
    _make_records(str(d / "val.tfrecords"), [(320, 420, []), (300, 300, []), (412, 412, [])])      # patches: 2+1, 2+1, 2+4 = 12
    net = Net(batch=4, input_size=299, k=5, mode="train")
    tr = Trainer(net, np.array(priors, np.float32), use_graph=False)
    CK.save(str(d / "log"), tr)
    del tr, net
    torch.cuda.empty_cache()
    return d


def _detect_cmd(d, out, *extra):
    return [sys.executable, os.path.join(ROOT, "detect.py"), "--priors", str(d / "priors.pkl"), "--checkpoint_path", str(d / "log"),
            "--config", str(d / "config.yaml"), "--save_dir", str(d / out), "--tfrecords", str(d / "val.tfrecords")] + list(extra)


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def cli_one_rank(cli_setup):
    d = cli_setup
    _run(_detect_cmd(d, "plain"))
    r = _run(_detect_cmd(d, "merged", "--merge_per_image", "--max_detections", "20"))
    return d, r.stdout


def test_cli_merge_per_image(cli_one_rank):
    d, stdout = cli_one_rank
    dense = open(d / "merged" / "results-dense-0.json", "rb").read()
    assert dense == open(d / "plain" / "results-dense-0.json", "rb").read()      # the dense file does not change
    assert not os.path.exists(d / "plain" / "results-merged-0.json")
    assert "results-merged-0.json" in stdout
    recs = json.loads(dense)
    groups = []                                                           # consecutive image_id = one image
    for x in recs:
        if not groups or groups[-1][0] != x["image_id"]:
            groups.append((x["image_id"], []))
        groups[-1][1].append(x)
    assert [gid for gid, _ in groups] == [1000, 1001, 1002]
    want = []
    for gid, xs in groups:
        s = np.array([x["score"] for x in xs], np.float32)
        assert [float(v) for v in s] == [x["score"] for x in xs]           # JSON round-trips the float32 scores exactly
        b = np.array([x["bbox"] for x in xs], np.float64)
        order = np.argsort(-s, kind="stable")[:16384]
        keep = order[nms_first(b[order], 0.5, 20)]
        assert len(xs) > 20 and 0 < len(keep) <= 20
        want += [{"image_id": gid, "bbox": b[k].tolist(), "score": float(s[k])} for k in keep]
    got = json.load(open(d / "merged" / "results-merged-0.json"))
    print("dense records", [len(xs) for _, xs in groups], "merged records", len(got))
    assert got == want


def test_cli_two_ranks_write_the_same_merged_file(cli_one_rank):
    """Two ranks on the one GPU: batch i belongs to rank i % 2, so every image's patches are split between them."""
    d, _ = cli_one_rank
    env = dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29531")
    cmd = _detect_cmd(d, "two", "--merge_per_image", "--max_detections", "20")
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(env, RANK=str(r)))
             for r in (0, 1)]
    outs, failed = [], False
    for p in procs:
        try:
            outs.append(p.communicate(timeout=30 if failed else 600)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
        failed = failed or p.returncode != 0
    assert not failed, "\n=====\n".join(o[-2000:] for o in outs)
    for name in ("results-merged-0.json", "results-dense-0.json"):
        assert open(d / "two" / name, "rb").read() == open(d / "merged" / name, "rb").read(), name
