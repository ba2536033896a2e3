"""mbx_coco_accumulate (the accumulation half of the COCO metric: global stable sort by score, running tp / fp per slice,
running maximum of the precision, lower bound per recall threshold), its host wrapper cocoeval.accumulate_device and
evaluate_bbox_device on top of both kernels, on the GPU.  The oracle is cocoeval.accumulate_tables (numpy) on the same
match arrays; every comparison is exact equality on float64."""
import numpy as np
import pytest

from multibox_amd import cocoeval as CE
from multibox_amd.synth import coco_eval_set

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
ALL, SMALL, MEDIUM, LARGE = range(4)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


def to_np(m):
    return tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in m)


def check(packed, m=None):
    """accumulate_device against accumulate_tables on the same match arrays (match_device's unless given)."""
    if m is None:
        m = CE.match_device(packed, on_device=True)
    precision, recall = CE.accumulate_device(packed, *m)
    want_p, want_r = CE.accumulate_tables(packed, *to_np(m))
    assert precision.dtype == recall.dtype == np.float64 and precision.shape == want_p.shape and recall.shape == want_r.shape
    for mi, md in enumerate(CE.MAX_DETS):                                            # a failure names the column
        assert np.array_equal(recall[:, :, mi], want_r[:, :, mi]), "recall, maxDets=%d" % md
        assert np.array_equal(precision[:, :, :, mi], want_p[:, :, :, mi]), "precision, maxDets=%d" % md
    return precision, recall


def subset(packed, images, last=None):
    """The images `images` of packed; `last`: only that many detections of the last one."""
    dt = [packed.dt[packed.dt_rows[i]:packed.dt_rows[i + 1]] for i in images]
    gt = [packed.gt[packed.gt_rows[i]:packed.gt_rows[i + 1]] for i in images]
    if last is not None:
        dt[-1] = dt[-1][:last]
    rows = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 5))
    return CE.Packed([packed.img_ids[i] for i in images], cat(dt), rows(dt), cat(gt), rows(gt))


# ---- 1. the three inputs of tests/test_cocoaccum_cpu.py
@pytest.mark.parametrize("seed,kw", [(21, {}), (22, dict(score_levels=0))])
def test_tables_equal_tied_and_continuous_scores(seed, kw):
    packed = CE.pack(*coco_eval_set(seed, 48, **kw))
    precision, recall = check(packed)
    assert (precision >= 0).all() and (recall >= 0).all() and (recall[:, :, 2] > 0).all()
    m = to_np(CE.match_device(packed))
    check(packed, m)                                                                 # numpy arrays instead of device tensors
    check(packed, (m[0] >= 0, m[1], m[2]))                                           # and match_host's bool `matched`


def test_tables_equal_with_empty_area_range():
    gt, dt = coco_eval_set(23, 24)
    packed = CE.pack([a for a in gt if a["area"] > 32.0 ** 2], dt)
    precision, recall = check(packed)
    assert (recall[:, SMALL, :] == -1).all() and int((recall == -1).sum()) == 30
    assert (precision[:, :, SMALL, :] == -1).all() and int((precision == -1).sum()) == 30 * len(CE.REC_THRS)


# ---- 2. many chunks and sort tiles
@pytest.fixture(scope="module")
def large():
    gt, dt = coco_eval_set(31, 700)
    packed = CE.pack(gt, dt)
    assert 40000 < len(packed.dt) < 50000
    return gt, dt, packed


def test_many_chunks_and_tiles(large):
    gt, dt, packed = large
    m = CE.match_device(packed)
    check(packed, m)
    out = CE.evaluate_bbox_device(gt, dt)
    print(len(packed.dt), out[0])
    assert out == CE.accumulate(packed, *m) and out[0][0] > 0.0


# ---- 3. ND around the chunk and the sort tile
ND_SWEEP = sorted({1, 63, 64, 65, CE.ACC_CHUNK - 1, CE.ACC_CHUNK, CE.ACC_CHUNK + 1, 2 * CE.ACC_CHUNK + 1, CE.ACC_SORT_TILE - 1,
                   CE.ACC_SORT_TILE, CE.ACC_SORT_TILE + 1, 2 * CE.ACC_SORT_TILE + 1})


@pytest.mark.parametrize("nd", ND_SWEEP)
def test_number_of_detections(large, nd):
    packed = large[2]
    k = int(np.searchsorted(packed.dt_rows, nd, side="left"))                        # images 0 .. k-1 hold at least nd
    sub = subset(packed, list(range(k)), last=nd - int(packed.dt_rows[k - 1]))
    assert len(sub.dt) == nd == sub.dt_rows[-1]
    check(sub)


# ---- 4. slots around the maxDets values
def test_slot_boundaries():
    counts = [(g, d) for d in (0, 1, 2, 10, 11, 100, 130) for g in (0, 2, 5, 9) if g or d]   # (pack has no image for 0 / 0)
    order = np.random.RandomState(3).permutation(len(counts))
    counts = [counts[k] for k in order]
    packed = CE.pack(*coco_eval_set(9, len(counts), counts=counts))
    assert np.diff(packed.dt_rows).tolist() == [min(c[1], 100) for c in counts]
    precision, recall = check(packed)
    assert not np.array_equal(recall[:, :, 0], recall[:, :, 1]) and not np.array_equal(recall[:, :, 1], recall[:, :, 2])


# ---- 5. hand cases
def box(image_id, x, y, w, h):
    return {"image_id": image_id, "bbox": [x, y, w, h], "area": w * h}


def hand(gt, dt):
    packed = CE.pack(gt, dt)
    return check(packed)


def test_equal_scores_keep_the_input_order():
    gt = [box(1, 0, 0, 50, 50), box(2, 0, 0, 50, 50), box(3, 0, 0, 50, 50)]
    dt = [[1, 200, 200, 50, 50, 0.5, 1], [2, 0, 0, 50, 50, 0.5, 1], [3, 200, 200, 50, 50, 0.5, 1]]     # fp, tp, fp
    precision, recall = hand(gt, dt)
    # tp 0 1 1, fp 1 1 2, npig 3: rc 0 1/3 1/3, pr 0 1/2 1/3 -> 1/2 1/2 1/3 from the right
    want = np.where(CE.REC_THRS <= 1.0 / 3.0, 1.0 / (2.0 + EPS), 0.0)
    assert want[33] == 0.5 and want[34] == 0.0
    for a in (ALL, MEDIUM):
        for mi in range(3):
            assert np.array_equal(precision[0, :, a, mi], want) and recall[0, a, mi] == 1.0 / 3.0
    assert (recall[:, (SMALL, LARGE), :] == -1).all() and (precision[:, :, (SMALL, LARGE), :] == -1).all()


def test_minus_zero_and_zero_scores_are_equal():
    gt = [box(1, 0, 0, 50, 50), box(2, 0, 0, 50, 50)]
    dt = [[1, 200, 200, 50, 50, -0.0, 1], [2, 0, 0, 50, 50, 0.0, 1]]                 # fp first: -0.0 does not sort after 0.0
    packed = CE.pack(gt, dt)
    assert np.signbit(packed.dt[0, 4]) and not np.signbit(packed.dt[1, 4])
    precision, recall = check(packed)
    # tp 0 1, fp 1 1, npig 2: rc 0 1/2, pr 0 1/2 -> 1/2 1/2
    want = np.where(CE.REC_THRS <= 0.5, 1.0 / (2.0 + EPS), 0.0)
    assert np.array_equal(precision[0, :, ALL, 2], want) and want[50] == 0.5 and want[51] == 0.0 and recall[0, ALL, 2] == 0.5


def test_gts_without_any_detection():
    precision, recall = hand([box(1, 0, 0, 50, 50), box(2, 0, 0, 20, 20)], [])
    assert (recall[:, (ALL, SMALL, MEDIUM), :] == 0).all() and (precision[:, :, (ALL, SMALL, MEDIUM), :] == 0).all()
    assert (recall[:, LARGE, :] == -1).all() and (precision[:, :, LARGE, :] == -1).all()


def test_recall_exactly_one_fills_the_last_threshold():
    precision, recall = hand([box(1, 0, 0, 50, 50)], [[1, 0, 0, 50, 50, 0.9, 1]])
    assert CE.REC_THRS[-1] == 1.0 and (recall[:, ALL, :] == 1.0).all()
    assert (precision[:, :, ALL, :] == 1.0 / (1.0 + EPS)).all() and 1.0 / (1.0 + EPS) == 0.9999999999999998


def test_recall_below_one_leaves_trailing_zeros():
    precision, recall = hand([box(1, 0, 0, 50, 50), box(1, 100, 100, 50, 50)], [[1, 0, 0, 50, 50, 0.9, 1]])
    assert (recall[:, ALL, :] == 0.5).all()
    want = np.where(CE.REC_THRS <= 0.5, 1.0 / (1.0 + EPS), 0.0)
    assert (precision[:, :, ALL, :] == want[None, :, None]).all() and want[51:].sum() == 0.0 and want[50] > 0.99


# ---- 6. the entry point itself
def raw_call(lib, packed, m, T=None, A=None, R=None, M=None, I=None, ws=None, ws_short=0, dt_rows=None):
    """(rc, precision, recall), the outputs pre-filled with 7.  T / A / R / M: the sizes passed, whatever the arrays hold."""
    import torch
    I = len(packed.img_ids) if I is None else I
    T, A = len(CE.IOU_THRS) if T is None else T, len(CE.AREA_RNG) if A is None else A
    R, M = len(CE.REC_THRS) if R is None else R, len(CE.MAX_DETS) if M is None else M
    thrs = np.ascontiguousarray(np.resize(CE.REC_THRS, max(R, 1)), np.float64)
    mds = np.ascontiguousarray(np.resize(CE.MAX_DETS, max(M, 1)), np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1) if a.size else np.zeros(1, a.dtype)).cuda()
    match, ignore, n_gt = to_np(m)
    ins = [dev(packed.dt), dev(packed.dt_rows if dt_rows is None else dt_rows), dev(match), dev(ignore), dev(n_gt)]
    o_p = torch.full((max(T, 1) * max(R, 1) * max(A, 1) * max(M, 1),), 7.0, dtype=torch.float64, device="cuda")
    o_r = torch.full((max(T, 1) * max(A, 1) * max(M, 1),), 7.0, dtype=torch.float64, device="cuda")
    nd = int(packed.dt_rows[-1])
    need = lib.mbx_coco_accumulate_workspace(nd, len(CE.IOU_THRS), len(CE.AREA_RNG), len(CE.MAX_DETS))
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.numel() >= need
    rc = lib.mbx_coco_accumulate(ins[0].data_ptr(), ins[1].data_ptr(), I, ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(), T, A,
                                 thrs.ctypes.data, R, mds.ctypes.data, M, o_p.data_ptr(), o_r.data_ptr(), ws.data_ptr(),
                                 need - ws_short if ws_short else ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, o_p.cpu().numpy(), o_r.cpu().numpy()


@pytest.fixture(scope="module")
def small():
    packed = CE.pack(*coco_eval_set(21, 48))
    return packed, CE.match_device(packed)


def test_no_image(lib, small):
    packed, m = small
    rc, precision, recall = raw_call(lib, packed, m, I=0)
    assert rc == 0 and (precision == -1).all() and (recall == -1).all()              # MBX_OK, tables of -1


def test_bad_sizes_leave_the_outputs_alone(lib, small):
    packed, m = small
    rc, precision, recall = raw_call(lib, packed, m)
    want_p, want_r = CE.accumulate_tables(packed, *m)
    assert rc == 0 and np.array_equal(precision.reshape(want_p.shape), want_p) and np.array_equal(recall.reshape(want_r.shape), want_r)
    for kw in (dict(R=129), dict(R=0), dict(M=5), dict(M=0), dict(T=17), dict(T=0), dict(A=9), dict(A=0), dict(ws_short=1)):
        rc, precision, recall = raw_call(lib, packed, m, **kw)
        assert rc == -1 and (precision == 7).all() and (recall == 7).all(), kw       # MBX_ERR_INVALID_ARG


def test_too_many_detections_is_refused_before_any_read(lib, small):
    packed, m = small
    one = subset(packed, [0])
    claim = np.array([0, CE.ACC_MAX_ND + 1], np.int32)                               # dt itself holds image 0's few rows
    rc, precision, recall = raw_call(lib, one, tuple(a[:1] for a in m), dt_rows=claim)
    assert rc == -2 and (precision == 7).all() and (recall == 7).all()               # MBX_ERR_UNSUPPORTED


@pytest.mark.parametrize("T,A", [(1, 1), (16, 8)])
def test_other_numbers_of_thresholds_and_ranges(monkeypatch, T, A):
    """One flag word of one bit and four full ones, on the six-image subset of test_gpu_cocomatch's test of that name."""
    monkeypatch.setattr(CE, "IOU_THRS", np.linspace(0.3, 0.9, T) if T > 1 else np.array([0.5]))
    monkeypatch.setattr(CE, "AREA_RNG", [(0.0, 1e10), (0.0, 400.0), (400.0, 1600.0), (1600.0, 6400.0), (6400.0, 1e10), (100.0, 100.0),
                                         (0.0, 0.0), (5e4, 1e10)][:A])
    counts = [(13, 65), (65, 100), (128, 130), (129, 1), (0, 63), (1, 1)]
    packed = CE.pack(*coco_eval_set(7, len(counts), counts=counts))
    precision, recall = check(packed)
    assert precision.shape == (T, 101, A, 3) and (recall[:, 0, :] >= 0).all() and recall[0, 0, 2] > 0


# ---- 7. an image mbx_coco_match refuses, inside a device-resident run
def test_refused_image_in_a_device_resident_run():
    counts = [(5, 20), (3, 0), (129, 30), (0, 7), (8, 100)]
    gt, dt = coco_eval_set(13, len(counts), counts=counts)
    packed = CE.pack(gt, dt)
    m = CE.match_device(packed, on_device=True)
    assert all(hasattr(t, "is_cuda") and t.is_cuda for t in m)
    host = CE.match_device(packed)
    assert all(np.array_equal(a, b) for a, b in zip(to_np(m), host)) and (host[0][2] >= 0).any() and host[2][2, 0] == 129
    assert CE.evaluate_bbox_device(gt, dt) == CE.evaluate_bbox(gt, dt)


# ---- 8. no state survives in the workspace
def test_two_calls_on_one_workspace(lib, small, large):
    import torch
    packed_a, m_a = small
    packed_b = subset(large[2], list(range(100, 160)))
    m_b = CE.match_device(packed_b)
    need = max(lib.mbx_coco_accumulate_workspace(len(p.dt), 10, 4, 3) for p in (packed_a, packed_b))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    for packed, m in ((packed_b, m_b), (packed_a, m_a), (packed_b, m_b)):
        rc, precision, recall = raw_call(lib, packed, m, ws=ws)
        want_p, want_r = CE.accumulate_tables(packed, *m)
        assert rc == 0 and np.array_equal(precision.reshape(want_p.shape), want_p) and np.array_equal(recall.reshape(want_r.shape), want_r)


def test_above_the_cap_numpy_accumulates(monkeypatch, small):
    """evaluate_bbox_device when accumulate_device refuses the size (the wrapper's own check, with the cap lowered)."""
    gt, dt = coco_eval_set(21, 48)
    packed, m = small
    monkeypatch.setattr(CE, "ACC_MAX_ND", 100)
    with pytest.raises(CE.AccumulateUnsupported):
        CE.accumulate_device(packed, *m)
    assert CE.evaluate_bbox_device(gt, dt) == CE.accumulate(packed, *m)
