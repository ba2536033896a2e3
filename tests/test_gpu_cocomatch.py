"""mbx_coco_match (matching of detections to ground truth for the COCO metric), its host wrapper
multibox_amd.cocoeval.match_device / evaluate_bbox_device and eval.py --device_metric, on the GPU.  The oracle is
cocoeval.match_host (_evaluate_img, the pure-Python restatement of pycocotools' evaluateImg) and evaluate_bbox; every
comparison is exact equality."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from multibox_amd import cocoeval as CE
from multibox_amd.synth import coco_eval_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG = """
NUM_BBOXES_PER_CELL : 5
MAX_NUM_BBOXES : 13
LOCATION_LOSS_ALPHA : 1000.0
BATCH_SIZE : 4
INPUT_SIZE : 299
NUM_TRAIN_EXAMPLES : 56945
NUM_TRAIN_ITERATIONS : 1000000
LOG_EVERY_N_STEPS : 1
BATCHNORM_MOVING_AVERAGE_DECAY : 0.3
INITIAL_LEARNING_RATE : 0.00001
DETECTION :
  USE_ORIGINAL_IMAGE : true
  ORIGINAL_IMAGE_MAX_TO_KEEP : 200
"""

N_DT = [0, 1, 63, 64, 65, 100, 130]                    # 130 is cut to 100 by pack
N_GT = [0, 1, 13, 64, 65, 128, 129]                    # 129: status 1, that image comes from the host
COUNTS = [(g, d) for g in N_GT for d in N_DT if g or d]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def mixed():
    """One image per pair of counts, in a shuffled order; (packed, counts per image, the oracle's three arrays)."""
    order = np.random.RandomState(5).permutation(len(COUNTS))
    counts = [COUNTS[k] for k in order]
    packed = CE.pack(*coco_eval_set(7, len(counts), counts=counts))
    assert np.diff(packed.gt_rows).tolist() == [c[0] for c in counts]
    assert np.diff(packed.dt_rows).tolist() == [min(c[1], 100) for c in counts]
    return packed, counts, CE.match_host(packed)


def subset(packed, images):
    dt = [packed.dt[packed.dt_rows[i]:packed.dt_rows[i + 1]] for i in images]
    gt = [packed.gt[packed.gt_rows[i]:packed.gt_rows[i + 1]] for i in images]
    rows = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 5))
    return CE.Packed([packed.img_ids[i] for i in images], cat(dt), rows(dt), cat(gt), rows(gt))


def check(packed, oracle):
    """match_device against the oracle's arrays, and what a named gt row must satisfy."""
    match, ignore, n_gt = CE.match_device(packed)
    matched, want_ignore, want_n = oracle
    I, A, T = len(packed.img_ids), len(CE.AREA_RNG), len(CE.IOU_THRS)
    assert match.shape == ignore.shape == (I, A, T, 100) and match.dtype == np.int16 and ignore.dtype == np.uint8
    assert n_gt.shape == (I, A) and n_gt.dtype == np.int32
    assert np.array_equal(match >= 0, matched)
    assert np.array_equal(ignore, want_ignore)
    assert np.array_equal(n_gt, want_n)
    for i in range(I):
        d, g = CE._image(packed, i)
        iou = CE._iou_xywh(d[:, :4], g[:, :4])
        assert (match[i, :, :, len(d):] == -1).all() and (match[i] >= -1).all() and (match[i] < len(g)).all()
        for ai in range(A):
            for ti, t in enumerate(CE.IOU_THRS):
                rows = match[i, ai, ti, :len(d)].astype(int)
                hit = np.nonzero(rows >= 0)[0]
                assert (iou[hit, rows[hit]] >= min(t, 1 - 1e-10)).all()
                assert len(set(rows[hit].tolist())) == len(hit)                      # no gt is named twice
    return match, ignore, n_gt


def test_all_counts_in_one_call(mixed):
    packed, counts, oracle = mixed
    match, ignore, n_gt = check(packed, oracle)
    print("matched", int((match >= 0).sum()), "ignored", int(ignore.sum()), "in-range gts", n_gt.sum(0).tolist())
    assert (match >= 0).sum() > 10000 and ignore.sum() > 10000                      # the comparison is not of empty arrays
    assert (match >= 64).any()                                                       # gts of the second half of a wave's lanes


@pytest.mark.parametrize("n_dt", N_DT)
def test_detection_counts(mixed, n_dt):
    packed, counts, oracle = mixed
    images = [i for i, c in enumerate(counts) if c[1] == n_dt]
    assert len(images) >= 6
    check(subset(packed, images), tuple(a[images] for a in oracle))


@pytest.mark.parametrize("n_gt", N_GT)
def test_gt_counts(mixed, n_gt):
    packed, counts, oracle = mixed
    images = [i for i, c in enumerate(counts) if c[0] == n_gt]
    assert len(images) >= 6
    check(subset(packed, images), tuple(a[images] for a in oracle))


def box(image_id, x, y, w, h, area=None):
    return {"image_id": image_id, "bbox": [x, y, w, h], "area": w * h if area is None else area}


HAND_GT = [box(1, 0, 0, 10, 10), box(2, 0, 0, 20, 20),                               # exact-threshold IoUs
           box(3, 50, 50, 40, 60), box(3, 50, 50, 40, 60),                           # duplicate gts
           box(4, 10, 10, 100, 100),                                                 # duplicate detections
           box(5, 0, 0, 32, 32), box(5, 100, 100, 96, 96),                           # areas exactly 32^2 and 96^2
           box(6, 0, 0, 40, 40), box(6, 0, 0, 30, 30),                               # medium around small
           box(7, 0, 0, 20, 20)]
HAND_DT = [[1, 0, 0, 10, 5, 0.9, 1],                                                 # IoU 50 / 100 = 0.5 exactly
           [2, 0, 0, 20, 15, 0.9, 1],                                                # IoU 300 / 400 = 0.75 exactly
           [3, 50, 50, 40, 60, 0.9, 1], [3, 50, 50, 40, 60, 0.8, 1], [3, 50, 50, 40, 60, 0.7, 1],
           [4, 10, 10, 100, 100, 0.9, 1], [4, 10, 10, 100, 100, 0.9, 1],
           [5, 0, 0, 32, 32, 0.9, 1], [5, 100, 100, 96, 96, 0.8, 1],
           [6, 0, 0, 40, 40, 0.9, 1],                                                # IoU 1 with the 40 x 40, 0.5625 with the 30 x 30
           [7, 150, 150, 100, 100, 0.9, 1]]                                          # far from its gt, large


def test_hand_cases():
    packed = CE.pack(HAND_GT, HAND_DT)
    assert packed.img_ids == [1, 2, 3, 4, 5, 6, 7]
    match, ignore, n_gt = check(packed, CE.match_host(packed))
    ALL, SMALL, MEDIUM, LARGE = range(4)
    assert CE.IOU_THRS[0] == 0.5 and match[0, ALL, 0, 0] == 0 and (match[0, ALL, 1:, 0] == -1).all()
    want75 = [0 if 0.75 >= t else -1 for t in CE.IOU_THRS]                           # IOU_THRS as passed, not 0.75 recomputed
    assert match[1, ALL, :, 0].tolist() == want75 and sum(want75) > -10
    # duplicate gts: equal IoUs -> the later gt; the next detection takes the other, a third none
    assert (match[2, ALL, :, :3] == [1, 0, -1]).all()
    # duplicate detections: the second is unmatched (input order among equal scores)
    assert (match[3, ALL, :, :2] == [0, -1]).all() and (ignore[3, LARGE, :, :2] == 0).all()
    # 32^2 is small AND medium, 96^2 medium AND large
    assert n_gt[4].tolist() == [2, 1, 2, 1]
    assert (ignore[4, SMALL, :, :2] == [0, 1]).all() and (ignore[4, MEDIUM, :, :2] == 0).all() and (ignore[4, LARGE, :, :2] == [1, 0]).all()
    # the in-range gt wins although the out-of-range one has the larger IoU; past IoU 0.5625 only the out-of-range one is left
    assert match[5, SMALL, :2, 0].tolist() == [1, 1] and (ignore[5, SMALL, :2, 0] == 0).all()
    assert (match[5, SMALL, 2:, 0] == 0).all() and (ignore[5, SMALL, 2:, 0] == 1).all()
    assert (match[5, MEDIUM, :, 0] == 0).all() and (ignore[5, MEDIUM, :, 0] == 0).all()
    # unmatched: ignored exactly where its own area (10 000) is out of range
    assert (match[6] == -1).all() and ignore[6, :, 0, 0].tolist() == [0, 1, 1, 0]


@pytest.mark.parametrize("seed", [11, 12])
def test_evaluate_bbox_device_equals_evaluate_bbox(seed):
    gt, dt = coco_eval_set(seed, 40)
    stats, lines = CE.evaluate_bbox_device(gt, dt)
    want_stats, want_lines = CE.evaluate_bbox(gt, dt)
    print(seed, want_stats)
    assert stats == want_stats and lines == want_lines and want_stats[0] > 0.0


def raw_call(lib, packed, thrs, rng, I=None):
    """The entry point itself; (rc, match, ignore, n_gt_counted, status), the outputs pre-filled with 7."""
    import torch
    I = len(packed.img_ids) if I is None else I
    thrs, rng = np.ascontiguousarray(thrs, np.float64), np.ascontiguousarray(rng, np.float64)
    T, A = len(thrs), len(rng)
    dev = lambda a: torch.from_numpy(a.reshape(-1) if a.size else np.zeros(1, a.dtype)).cuda()
    ins = [dev(a) for a in (packed.dt, packed.dt_rows, packed.gt, packed.gt_rows)]
    n = max(I, 1)
    outs = [torch.full((n, A, T, 100), 7, dtype=torch.int16, device="cuda"), torch.full((n, A, T, 100), 7, dtype=torch.uint8, device="cuda"),
            torch.full((n, A), 7, dtype=torch.int32, device="cuda"), torch.full((n,), 7, dtype=torch.int32, device="cuda")]
    rc = lib.mbx_coco_match(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), I, thrs.ctypes.data, T,
                            rng.ctypes.data, A, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in outs)


def test_no_image_and_bad_sizes(lib):
    packed = CE.pack(HAND_GT, HAND_DT)
    rc, match, ignore, n_gt, status = raw_call(lib, packed, CE.IOU_THRS, CE.AREA_RNG, I=0)
    assert rc == 0 and (match == 7).all() and (status == 7).all()                    # MBX_OK, nothing launched
    for thrs, rng in ((np.linspace(0.1, 0.9, 17), CE.AREA_RNG), (CE.IOU_THRS, [(0.0, 1e10)] * 9), (CE.IOU_THRS[:0], CE.AREA_RNG)):
        rc, match, _, _, status = raw_call(lib, packed, thrs, rng)
        assert rc == -1 and (match == 7).all() and (status == 7).all()               # MBX_ERR_INVALID_ARG


def test_status_and_outputs_of_a_refused_image(lib, mixed):
    """More than 128 gts: status 1 and -1 / 0 / 0 from the kernel (match_device then takes the image from the host)."""
    packed, counts, _ = mixed
    rc, match, ignore, n_gt, status = raw_call(lib, packed, CE.IOU_THRS, CE.AREA_RNG)
    assert rc == 0 and status.tolist() == [int(c[0] > 128) for c in counts] and status.sum() == len(N_DT)
    bad = status == 1
    assert (match[bad] == -1).all() and (ignore[bad] == 0).all() and (n_gt[bad] == 0).all()


@pytest.mark.parametrize("T,A", [(1, 1), (16, 8)])
def test_other_numbers_of_thresholds_and_ranges(monkeypatch, mixed, T, A):
    """The workgroup has one wavefront per threshold: the smallest and the largest one, against the same oracle."""
    monkeypatch.setattr(CE, "IOU_THRS", np.linspace(0.3, 0.9, T) if T > 1 else np.array([0.5]))
    monkeypatch.setattr(CE, "AREA_RNG", [(0.0, 1e10), (0.0, 400.0), (400.0, 1600.0), (1600.0, 6400.0), (6400.0, 1e10), (100.0, 100.0),
                                         (0.0, 0.0), (5e4, 1e10)][:A])
    packed, counts, _ = mixed
    images = [i for i, c in enumerate(counts) if c in ((13, 65), (65, 100), (128, 130), (129, 1), (0, 63), (1, 1))]
    assert len(images) == 6
    sub = subset(packed, images)
    check(sub, CE.match_host(sub))


def test_nan_score_takes_the_host_path(capfd):
    dt = [list(r) for r in HAND_DT]
    dt[2][5] = float("nan")
    packed = CE.pack(HAND_GT, dt)
    match, ignore, n_gt = CE.match_device(packed)
    assert "WARNING: non-finite" in capfd.readouterr().err
    matched, want_ignore, want_n = CE.match_host(packed)
    assert np.array_equal(match >= 0, matched) and np.array_equal(ignore, want_ignore) and np.array_equal(n_gt, want_n)
    assert (match[2, 0, :, :3] == [1, 0, -1]).all()                                  # the rows are still named


def test_eval_cli_device_metric(tmp_path):
    """eval.py --device_metric end to end, on the records and the checkpoint recipe of test_gpu_cli.test_eval_cli."""
    import __graft_entry__ as g
    g.build()
    import torch
    from multibox_amd import priors as PR, checkpoint as CK
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer
    from tests.test_inputs_cpu import _make_records
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CFG)
    pri = tmp_path / "priors.pkl"
    priors = PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.])
    PR.save_priors(str(pri), priors)
    rec = str(tmp_path / "val.tfrecords")
    _make_records(rec, [(320, 420, [[.1, .1, .6, .7]]), (300, 300, []), (412, 412, [[.2, .3, .9, .8], [.0, .0, .3, .3]]),
                        (299, 299, [[.4, .4, .6, .6]]), (310, 330, [[.1, .1, .2, .2]])])            # 5 images: one batch of 4
    net = Net(batch=4, input_size=299, k=5, mode="train")
    tr = Trainer(net, np.array(priors, np.float32), use_graph=False)
    CK.save(str(tmp_path / "log"), tr)
    del tr, net
    torch.cuda.empty_cache()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--priors", str(pri), "--checkpoint_path", str(tmp_path / "log"),
                        "--config", str(cfg), "--summary_dir", str(tmp_path / "sum"), "--tfrecords", rec, "--device_metric"],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.load(open(tmp_path / "sum" / "eval-0.json"))
    assert out["metric_path"] == "device" and out["images"] == 4 and len(out["stats"]) == 12 and len(out["summary"]) == 12
    assert all(-1.0 <= v <= 1.0 for v in out["stats"]) and out["stats"][0] >= 0.0
