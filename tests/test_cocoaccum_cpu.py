"""cocoeval.accumulate_tables (the numpy restatement of COCOeval.accumulate that mbx_coco_accumulate is held against) and the
plumbing of the new entry points, without a GPU.  Every comparison is exact equality."""
import os
import re

import numpy as np
import pytest

from multibox_amd import cocoeval as CE
from multibox_amd.synth import coco_eval_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed,kw,nd", [(21, {}, 2292), (22, dict(score_levels=0), 2871)])
def test_tables_then_summary_equal_accumulate_equal_evaluate_bbox(seed, kw, nd):
    gt, dt = coco_eval_set(seed, 48, **kw)
    packed = CE.pack(gt, dt)
    assert len(packed.dt) == nd
    m = CE.match_host(packed)
    precision, recall = CE.accumulate_tables(packed, *m)
    T, R, A, M = len(CE.IOU_THRS), len(CE.REC_THRS), len(CE.AREA_RNG), len(CE.MAX_DETS)
    assert precision.shape == (T, R, A, M) and recall.shape == (T, A, M) and precision.dtype == recall.dtype == np.float64
    assert (precision >= 0).all() and (recall >= 0).all()                            # no -1 slice
    want = CE.evaluate_bbox(gt, dt)
    print(seed, want[0])
    assert CE._summarize(precision, recall) == CE.accumulate(packed, *m) == want
    assert 0.15 < want[0][0] < 0.25


def test_area_range_without_gt_stays_minus_one():
    gt, dt = coco_eval_set(23, 24)
    gt = [a for a in gt if a["area"] > 32.0 ** 2]
    packed = CE.pack(gt, dt)
    precision, recall = CE.accumulate_tables(packed, *CE.match_host(packed))
    small = CE.AREA_LBL.index("small")
    assert (recall[:, small, :] == -1).all() and int((recall == -1).sum()) == 30
    assert (precision[:, :, small, :] == -1).all() and int((precision == -1).sum()) == 30 * len(CE.REC_THRS)
    assert CE._summarize(precision, recall) == CE.evaluate_bbox(gt, dt)


def test_new_symbols_are_declared():
    from multibox_amd import _lib
    assert "mbx_coco_accumulate" in _lib.declared_symbols() and "mbx_coco_accumulate_workspace" in _lib.declared_symbols()


def test_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "mbx.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert CE.ACC_MAX_ND == value("MBX_COCO_ACC_MAX_ND") >= 2000000
    assert CE.ACC_CHUNK == value("MBX_COCO_ACC_CHUNK") and CE.ACC_SORT_TILE == value("MBX_COCO_ACC_SORT_TILE")
    assert len(CE.REC_THRS) <= value("MBX_COCO_ACC_MAX_R") and len(CE.MAX_DETS) <= value("MBX_COCO_ACC_MAX_M")


def test_workspace_query():
    """Host-only: linear in ND with the header's constant, 0 outside the limits."""
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    ws = _lib.lib().mbx_coco_accumulate_workspace
    assert ws(0, 10, 4, 3) > 0
    for T, A, M, per in ((10, 4, 3, 48.5), (16, 8, 4, 89.0)):
        small, big = ws(1000, T, A, M), ws(2001000, T, A, M)
        assert 0 < small < big and abs((big - small) / 2e6 - per) < 0.1
    assert ws(CE.ACC_MAX_ND, 16, 8, 4) > 0 and ws(CE.ACC_MAX_ND + 1, 10, 4, 3) == 0 and ws(-1, 10, 4, 3) == 0
    assert ws(100, 17, 4, 3) == 0 and ws(100, 10, 9, 3) == 0 and ws(100, 10, 4, 5) == 0 and ws(100, 0, 4, 3) == 0
