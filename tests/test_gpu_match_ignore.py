"""GPU: mbx_match_ignore (the ignore band behind the matching) against tests/ignore_oracle.py.

The C ABI is driven directly with the hand-made `match` of tests/test_gpu_match_extend.make_case, so this half depends on no
matcher.  The bar is exactness: the kernel's float64 IoU has the oracle's operations in the oracle's order, so `match` and
`n_ignored` are compared bit for bit.  Shapes: fewer priors than one wavefront (13), a partial second wavefront (70), eleven
wavefronts of which the last is partial (646), and the strided loop of 1 024 threads with a tail (3 199).
"""
import functools

import numpy as np
import pytest

from tests import extend_oracle as EO
from tests import ignore_oracle as IO
from tests.loss_cases import gpu  # noqa: F401  (the fixture is found by name)
from tests.test_gpu_match_extend import SHAPES, make_case
from tests.test_gpu_match_extend import call as call_extend

pytestmark = pytest.mark.gpu

SENTINEL = -77
# the number ignored per image on the hand-made match at 0.5 (tests/test_ignore_cpu.py holds the oracle to the same table)
AT_HALF = {(3, 13, 13): [0, 6, 2], (4, 70, 5): [0, 7, 3, 1], (4, 646, 13): [0, 47, 3, 17], (2, 3199, 100): [0, 966]}


@functools.lru_cache(maxsize=None)
def jittered(B, P, G, grid=0):
    """[B,P,4]: the case's priors moved by up to 0.03 a coordinate, another draw per image -- what a decoded prediction looks
    like to the kernel; on a grid, by -1, 0 or 1 grid steps a coordinate (exact in float32)."""
    c = make_case(B, P, G, grid)
    rng = np.random.RandomState(31 * P + B)
    if grid:
        boxes = (c["priors"][None] + rng.randint(-1, 2, (B, P, 4)).astype(np.float32) / np.float32(grid)).astype(np.float32)
    else:
        boxes = (c["priors"][None] + rng.uniform(-0.03, 0.03, (B, P, 4))).astype(np.float32)
    boxes.setflags(write=False)
    return boxes


@functools.lru_cache(maxsize=None)
def oracle(B, P, G, thr, per_image=0, grid=0):
    c = make_case(B, P, G, grid)
    boxes = jittered(B, P, G, grid) if per_image else c["priors"]
    out, n = IO.ignore(boxes, per_image, c["gt"], c["n"], c["status"], c["match"], thr)
    out.setflags(write=False); n.setflags(write=False)
    return out, n


def call(gpu, c, thr, rows=None, with_count=True, null=None, per_image=0, boxes=None, **override):
    """One call of the C ABI on images `rows` of case c (arrays in `override` replace the case's; `boxes` defaults to the
    priors) -> (status, match [B,P], n_ignored [B] prefilled with SENTINEL).  null: the name of a pointer passed as NULL.
    B, P, G in `override` replace the sizes passed (for the refusals: nothing is launched)."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    get = lambda k: override.get(k, c[k])
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()                 # a copy: the case's arrays are read-only
    boxes = c["priors"] if boxes is None else boxes
    t = dict(boxes=dev(boxes[rows] if per_image else boxes), gt=dev(get("gt")[rows]), n=dev(get("n")[rows]),
             status=dev(get("status")[rows]), match=dev(get("match")[rows]))
    B, P = t["match"].shape
    n_ignored = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    ptr = lambda k: None if null == k else t[k].data_ptr()
    st = l.mbx_match_ignore(ptr("boxes"), per_image, ptr("gt"), ptr("n"), ptr("status"), float(thr), override.get("B", B),
                            override.get("P", P), override.get("G", c["G"]), ptr("match"),
                            n_ignored.data_ptr() if with_count else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, t["match"].cpu().numpy(), n_ignored.cpu().numpy()


# --------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("per_image", [0, 1])
@pytest.mark.parametrize("thr", [0.3, 0.5])
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_match_and_n_ignored_equal_the_oracle(gpu, B, P, G, thr, per_image):
    c = make_case(B, P, G)
    want, want_n = oracle(B, P, G, thr, per_image)
    assert want_n.sum() >= 1 and want_n[0] == 0                          # the case ignores something, or it shows nothing
    if thr == 0.5 and not per_image:
        assert want_n.tolist() == AT_HALF[(B, P, G)]
    st, match, n_ignored = call(gpu, c, thr, per_image=per_image, boxes=jittered(B, P, G) if per_image else None)
    print("ignored per image", n_ignored, "oracle", want_n)
    assert st == 0
    assert match.tobytes() == want.tobytes() and n_ignored.tobytes() == want_n.tobytes()
    stays = c["match"] != -1
    assert np.array_equal(match[stays], c["match"][stays])               # positives keep their box
    assert np.array_equal(n_ignored, ((match == -2) & (c["match"] == -1)).sum(1))


@pytest.mark.parametrize("B,P,G", SHAPES)
def test_entries_at_or_under_minus_two_and_positives_are_left_alone(gpu, B, P, G):
    c = make_case(B, P, G)
    match = c["match"].copy()
    free = np.nonzero(match.reshape(-1) == -1)[0]
    match.reshape(-1)[free[::3]] = -2                                    # a third of the free priors: ignored before, -3, -77
    match.reshape(-1)[free[1::7]] = -3
    match.reshape(-1)[free[2::11]] = -77
    want, want_n = IO.ignore(c["priors"], 0, c["gt"], c["n"], c["status"], match, 0.3)
    assert want_n.sum() >= 1
    st, out, n_ignored = call(gpu, c, 0.3, match=match)
    assert st == 0 and out.tobytes() == want.tobytes() and n_ignored.tobytes() == want_n.tobytes()
    stays = match != -1
    assert np.array_equal(out[stays], match[stays]) and (out[stays] <= -2).sum() > 0
    assert np.array_equal(n_ignored, ((out == -2) & (match == -1)).sum(1))       # what was -2 on input is not counted


@pytest.mark.parametrize("per_image", [0, 1])
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_quantised_coordinates_where_ious_are_exact(gpu, B, P, G, per_image):
    c = make_case(B, P, G, grid=16)
    boxes = jittered(B, P, G, 16) if per_image else c["priors"]
    # thresholds that IoUs of areas in 1/256 hit exactly: 0.25, 0.5, 0.75 are float32 numbers
    for thr in (0.25, 0.5, 0.75):
        want, want_n = oracle(B, P, G, thr, per_image, 16)
        assert want_n.sum() >= 1
        st, match, n_ignored = call(gpu, c, thr, per_image=per_image, boxes=boxes if per_image else None)
        assert st == 0 and match.tobytes() == want.tobytes() and n_ignored.tobytes() == want_n.tobytes()
    at = [(b, p) for b in range(B) for p in np.nonzero(c["match"][b] == -1)[0] if c["n"][b]
          and (EO.iou_row((boxes[b] if per_image else boxes)[p], c["gt"][b, :c["n"][b]]).max() == 0.5)]
    print("free priors whose largest IoU is exactly 0.5:", len(at))
    want, _ = oracle(B, P, G, 0.5, per_image, 16)
    assert all(want[b, p] == -2 for b, p in at)


def test_an_iou_of_exactly_the_threshold_is_ignored_and_the_next_float_is_not(gpu):
    c = dict(B=1, P=1, G=1, priors=np.array([[0, 0, .5, .5]], np.float32), gt=np.array([[[0, 0, .5, .25]]], np.float32),
             n=np.array([1], np.int32), status=np.zeros(1, np.int32), match=-np.ones((1, 1), np.int32))
    assert EO.iou_row(c["priors"][0], c["gt"][0])[0] == 0.5
    st, match, n_ignored = call(gpu, c, 0.5)
    assert st == 0 and match.tolist() == [[-2]] and n_ignored.tolist() == [1]
    st, match, n_ignored = call(gpu, c, np.nextafter(np.float32(0.5), np.float32(1)))
    assert st == 0 and match.tolist() == [[-1]] and n_ignored.tolist() == [0]
    st, match, n_ignored = call(gpu, c, 0.5, per_image=1, boxes=c["priors"][None])
    assert st == 0 and match.tolist() == [[-2]] and n_ignored.tolist() == [1]


@pytest.mark.parametrize("lo,hi", [(0.3, 0.5), (0.5, 0.5)])
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_the_band_is_the_complement_of_threshold_matching(gpu, B, P, G, lo, hi):
    c = make_case(B, P, G, grid=16 if lo == hi else 0)                   # lo == hi: the band is the IoUs of exactly hi
    st, ext, n_extra = call_extend(gpu, c, hi)
    assert st == 0
    st, band, n_ignored = call(gpu, c, lo, match=ext)
    assert st == 0
    best = IO.best_iou(c["priors"], c["gt"], c["n"])
    free = c["match"] < 0
    flo, fhi = float(np.float32(lo)), float(np.float32(hi))
    in_band = free & (best >= flo) & (best <= fhi)
    print("added", n_extra, "ignored", n_ignored, "in the band", in_band.sum(1))
    assert in_band.any() == ((B, P, G) != (3, 13, 13))                   # (3, 13, 13) is the "nothing to ignore" row
    assert np.array_equal(band == -2, in_band)                           # every one of them, and nothing else
    assert np.array_equal(band >= 0, ~free | (best > fhi))               # no prior is both
    assert np.array_equal(n_ignored, in_band.sum(1))


# ------------------------------------------------------------------------------------------------- what stays untouched
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_skipped_images_keep_their_row_byte_for_byte(gpu, B, P, G):
    c = make_case(B, P, G)
    want, want_n = oracle(B, P, G, 0.3)
    pattern = (np.arange(B * P, dtype=np.int32).reshape(B, P) % 5) - 3     # -3 .. 1: free, ignored and "matched" entries alike
    keep = [b for b in range(B) if b != 1]
    for what in ("status 1", "status 2", "n > G", "n = 0", "n < 0"):
        status, n = np.zeros(B, np.int32), c["n"].copy()
        if what.startswith("status"):
            status[1] = int(what[-1])
        else:
            n[1] = {"n > G": G + 1, "n = 0": 0, "n < 0": -4}[what]
        match = c["match"].copy()
        match[1] = pattern[1]
        st, out, n_ignored = call(gpu, c, 0.3, status=status, n=n, match=match)
        assert st == 0, what
        assert out[1].tobytes() == pattern[1].tobytes() and n_ignored[1] == 0, what
        assert out[0].tobytes() == c["match"][0].tobytes() and n_ignored[0] == 0         # n_gt = 0
        assert out[keep].tobytes() == want[keep].tobytes() and np.array_equal(n_ignored[keep], want_n[keep]), what


@pytest.mark.parametrize("B,P,G", SHAPES)
def test_a_nan_in_the_padding_rows_changes_nothing(gpu, B, P, G):
    c = make_case(B, P, G)
    want, want_n = oracle(B, P, G, 0.3)
    gt = c["gt"].copy()
    for b in range(B):
        gt[b, c["n"][b]:] = np.nan
    assert np.isnan(gt).any()
    st, match, n_ignored = call(gpu, c, 0.3, gt=gt)
    assert st == 0 and match.tobytes() == want.tobytes() and n_ignored.tobytes() == want_n.tobytes()


def test_non_finite_and_degenerate_boxes_follow_the_formula(gpu):
    c = make_case(4, 70, 5)
    boxes = jittered(4, 70, 5).copy()
    free = np.nonzero(c["match"][1] == -1)[0]
    boxes[1, free[0]] = np.nan
    boxes[1, free[1], 2] = np.inf
    boxes[1, free[2]] = boxes[1, free[2]][[2, 1, 0, 3]]                  # x1 > x2
    boxes[1, free[3], 2:] = boxes[1, free[3], :2]                        # a point
    boxes[1, free[4]] = c["gt"][1, 0]                                    # and one that sits on a box
    want, want_n = IO.ignore(boxes, 1, c["gt"], c["n"], c["status"], c["match"], 0.3)
    assert want[1, free[4]] == -2 and np.all(want[1, free[:4]] == -1)
    st, match, n_ignored = call(gpu, c, 0.3, per_image=1, boxes=boxes)
    assert st == 0 and match.tobytes() == want.tobytes() and n_ignored.tobytes() == want_n.tobytes()


# ------------------------------------------------------------------------------------- independence and reproducibility
@pytest.mark.parametrize("per_image", [0, 1])
@pytest.mark.parametrize("B,P,G", SHAPES)
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, B, P, G, per_image):
    c = make_case(B, P, G)
    kw = dict(per_image=per_image, boxes=jittered(B, P, G) if per_image else None)
    _, full, full_n = call(gpu, c, 0.3, **kw)
    _, again, again_n = call(gpu, c, 0.3, **kw)
    assert full.tobytes() == again.tobytes() and full_n.tobytes() == again_n.tobytes()
    st, twice, twice_n = call(gpu, c, 0.3, match=full, **kw)              # a second call on its own output: a no-op
    assert st == 0 and twice.tobytes() == full.tobytes() and not twice_n.any()
    st, no_count, untouched = call(gpu, c, 0.3, with_count=False, **kw)   # n_ignored = NULL
    assert st == 0 and no_count.tobytes() == full.tobytes() and np.all(untouched == SENTINEL)
    perm = np.arange(B)[::-1].copy()
    st, out, n = call(gpu, c, 0.3, rows=perm, **kw)
    assert st == 0 and out.tobytes() == full[perm].tobytes() and np.array_equal(n, full_n[perm])
    for b in range(B):
        st, out, n = call(gpu, c, 0.3, rows=slice(b, b + 1), **kw)
        assert st == 0 and out.tobytes() == full[b:b + 1].tobytes() and n[0] == full_n[b]


# --------------------------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("kw,status", [
    (dict(thr=0.0), -1), (dict(thr=-0.1), -1), (dict(thr=1.5), -1), (dict(thr=float("nan")), -1), (dict(thr=float("inf")), -1),
    (dict(thr=0.3, null="boxes"), -1), (dict(thr=0.3, null="gt"), -1), (dict(thr=0.3, null="n"), -1),
    (dict(thr=0.3, null="status"), -1), (dict(thr=0.3, null="match"), -1),
    (dict(thr=0.3, B=-1), -1), (dict(thr=0.3, P=0), -1), (dict(thr=0.3, P=-5), -1), (dict(thr=0.3, G=0), -1),
    (dict(thr=0.3, G=1537), -2), (dict(thr=0.3, G=1 << 20), -2)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, kw, status):
    c = make_case(4, 70, 5)
    sentinel = np.full((4, 70), SENTINEL, np.int32)
    for per_image in (0, 1):
        st, match, n_ignored = call(gpu, c, match=sentinel, per_image=per_image,
                                    boxes=jittered(4, 70, 5) if per_image else None, **kw)
        assert st == status
        assert np.all(match == SENTINEL) and np.all(n_ignored == SENTINEL)
    st, match, n_ignored = call(gpu, c, 0.3)                               # the same call with good arguments writes
    assert st == 0 and not np.any(n_ignored == SENTINEL)


def test_no_image_is_no_error_and_the_largest_g_is_taken(gpu):
    torch, l = gpu
    c = make_case(4, 70, 5)
    st, match, n_ignored = call(gpu, c, 0.3, B=0)
    assert st == 0 and match.tobytes() == c["match"].tobytes() and np.all(n_ignored == SENTINEL)
    # G = 1536, the most the LDS of a plain launch holds: the case's boxes in rows of 1536
    gt = np.zeros((4, 1536, 4), np.float32)
    gt[:, :5] = c["gt"]
    want, want_n = IO.ignore(c["priors"], 0, c["gt"], c["n"], c["status"], c["match"], 0.3)
    st, match, n_ignored = call(gpu, c, 0.3, gt=gt, G=1536)
    assert st == 0 and match.tobytes() == want.tobytes() and n_ignored.tobytes() == want_n.tobytes()


# ---------------------------------------------------------------------------------------------------------- the wrapper
def test_ignore_matches_wrapper(gpu):
    torch, _ = gpu
    from multibox_amd import _lib, loss as L
    c = make_case(4, 646, 13)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    for per_image in (0, 1):
        boxes = jittered(4, 646, 13) if per_image else c["priors"]
        want, want_n = oracle(4, 646, 13, 0.5, per_image)
        match, n_ignored = dev(c["match"]), torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
        out, n = L.ignore_matches(dev(boxes), dev(c["gt"]), dev(c["n"]), dev(c["status"]), match, 0.5, n_ignored)
        torch.cuda.synchronize()
        assert out is match and n is n_ignored
        assert match.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(n_ignored.cpu().numpy(), want_n)
    with pytest.raises(_lib.MbxError):
        L.ignore_matches(dev(c["priors"]), dev(c["gt"]), dev(c["n"]), dev(c["status"]), match, 0.0)
