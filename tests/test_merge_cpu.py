"""Host side of the per-image merge (mbx_merge_detections / ImageMerger): row grouping, the truncation of an oversize
image, the transport of rows between ranks, and the C-ABI tables.  No GPU."""
import os
import re

import numpy as np

from multibox_amd import records as REC
from multibox_amd.synth import merge_candidates
from tests.merge_oracle import CASES, candidate_order, merge_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_rows():
    ids, rows = REC.group_rows([7, 7, 7, 9, 8, 8])
    assert ids == [7, 9, 8] and rows.tolist() == [0, 3, 4, 6] and rows.dtype == np.int32
    ids, rows = REC.group_rows(["a", "a", "b", "a"])                     # an id that returns later is a new image
    assert ids == ["a", "b", "a"] and rows.tolist() == [0, 2, 3, 4]
    ids, rows = REC.group_rows([])
    assert ids == [] and rows.tolist() == [0]
    ids, rows = REC.group_rows([5])
    assert ids == [5] and rows.tolist() == [0, 1]
    # the padding rows of a partial batch repeat the last id (inputs.detect_batches) with count 0: they join that image
    ids, rows = REC.group_rows([1000, 1000, 1001] + [1001] * 5)
    assert ids == [1000, 1001] and rows.tolist() == [0, 2, 8]
    ids, rows = REC.group_rows(np.array([3, 3, 4]))
    assert [int(i) for i in ids] == [3, 4] and rows.tolist() == [0, 2, 3]


def test_generator_cases_are_what_the_issue_states():
    """The seeded cases cover both exits of the walk by the oracle alone (the cheap ones; the GPU test runs all five)."""
    for name, cands, kept in (("small", (7, 126), (4, 41)), ("topn", (127, 249), (100, 100))):
        kw, max_det, thr = CASES[name]
        b, s, c, ir = merge_candidates(**kw)
        n = [int(c[ir[i]:ir[i + 1]].sum()) for i in range(len(ir) - 1)]
        k = [len(o) for o in merge_oracle(b, s, c, ir, max_det, thr)]
        assert (min(n), max(n)) == cands and (min(k), max(k)) == kept, (name, n, k)


def test_truncation_keeps_the_oracles_first_16384_in_order():
    b, s, c, ir = merge_candidates(seed=11, I=1, rows_per_image=(100, 100), K=200, n_obj=10, count=200)
    c[::7] = 150                                                         # rows of different fill
    assert int(c.sum()) > REC.MERGE_MAX_CANDIDATES
    want = candidate_order(s, c, 0, len(c))
    got = REC.best_candidates(s, c)
    assert len(got) == REC.MERGE_MAX_CANDIDATES and np.array_equal(got, want)
    assert len(np.unique(s.reshape(-1)[got])) < 100                      # ties everywhere: the index rule decided
    # re-packed into rows of k_max slots, the device's order (score, then flat index) is the same list again
    nb, ns, nc = REC.repack_rows(b, s, got, 200)
    assert nb.shape == (82, 200, 4) and nc.tolist() == [200] * 81 + [184]
    again = candidate_order(ns, nc, 0, len(nc))
    assert np.array_equal(again, np.arange(REC.MERGE_MAX_CANDIDATES))
    assert nb.reshape(-1, 4)[:len(got)].tobytes() == b.reshape(-1, 4)[got].tobytes()
    assert ns.reshape(-1)[:len(got)].tobytes() == s.reshape(-1)[got].tobytes()
    # below the limit nothing is cut
    assert np.array_equal(REC.best_candidates(s[:10], c[:10]), candidate_order(s, c, 0, 10))


def test_score_order_keys_follow_the_device_rule():
    s = np.array([0.5, -0.0, 0.0, np.nan, -1.0, np.inf, -np.inf, 2.0, 1e-45], np.float32)
    k = REC.score_order_keys(s).astype(np.int64)
    assert k[1] == k[2]                                                  # -0 == +0
    assert k[3] == k.max() and (k[3] > np.delete(k, 3)).all()            # a NaN above everything
    finite = [0, 1, 4, 5, 6, 7, 8]
    assert np.array_equal(np.argsort(-k[finite], kind="stable"), np.argsort(-s[finite], kind="stable"))
    # ties: ascending flat index
    assert REC.best_candidates(np.array([[0.5, 0.25, 0.5], [0.5, 0.75, 0.0]], np.float32), [3, 2]).tolist() == [4, 0, 2, 3, 1]


def test_compact_expand_roundtrip():
    b, s, c, _ = merge_candidates(seed=3, I=2, rows_per_image=(3, 5), K=20, n_obj=3)
    c[0] = 0
    cnt, bv, sv = REC.compact_rows(b, s, c)
    assert len(bv) == len(sv) == int(c.sum())
    b2, s2, c2 = REC.expand_rows(cnt, bv, sv, 20)
    valid = np.arange(20)[None, :] < c[:, None]
    assert np.array_equal(c2, c) and b2[valid].tobytes() == b[valid].tobytes() and s2[valid].tobytes() == s[valid].tobytes()
    assert not b2[~valid].any() and not s2[~valid].any()


def test_merge_entry_point_is_declared():
    from multibox_amd import _lib
    assert "mbx_merge_detections" in _lib._SIGS
    res, args = _lib._SIGS["mbx_merge_detections"]
    assert len(args) == 14
    hdr = open(os.path.join(ROOT, "include", "mbx.h")).read()
    assert re.search(r"#define\s+MBX_MERGE_MAX_CANDIDATES\s+16384\b", hdr)
    assert re.search(r"\bint\s+mbx_merge_detections\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert REC.MERGE_MAX_CANDIDATES == 16384


def test_detect_cli_has_the_merge_flag():
    src = open(os.path.join(ROOT, "detect.py")).read()
    assert '"--merge_per_image"' in src and "results-merged-%d.json" in src and "MERGE_IOU_THRESHOLD" in src
