"""The oracle and the shared inputs of the edge tests of mbx_match, mbx_decode_filter_topk, mbx_nms and mbx_decode_conf
(tests/test_postproc_oracle_cpu.py, tests/test_gpu_postproc_edges.py).  numpy / float64 and what oracle/ has, no torch and
never the code under test.  The input builders are shared by both files so that the CPU tests prove, without a GPU, that
the reference alone meets the preconditions each case relies on."""
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

from oracle import ref_numpy as R

EPS = np.float32(1e-10)


def ulp32(x):
    """The spacing of float32 at |x|."""
    return float(np.spacing(np.float32(abs(float(x)))))


def costs(dec, conf, gt, n, alpha):
    """cost_matrix of one image without numpy's overflow warnings (a prediction at 1e20 has an infinite column on purpose)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return R.cost_matrix(dec, conf, gt[:n], alpha)


# ----------------------------------------------------------------------------------------------------------- assignment
def assignment_cost(C, match_row):
    """C [P, n] (oracle.ref_numpy.cost_matrix), match_row [P] = gt index or -1.  Asserts that the row is a valid assignment --
    every gt in [0, n) exactly once, on distinct predictions, everything else -1 -- and returns its total cost, summed with
    math.fsum so that the sum adds no rounding of its own."""
    P, n = C.shape
    m = np.asarray(match_row)
    assert m.shape == (P,), (m.shape, P)
    pos = np.nonzero(m >= 0)[0]
    assert (m[m < 0] == -1).all(), "entries other than a gt index or -1"
    assert sorted(m[pos].tolist()) == list(range(n)), "not every gt exactly once: %s" % sorted(m[pos].tolist())
    return math.fsum(float(C[p, m[p]]) for p in pos)


def scipy_total(C):
    rows, cols = linear_sum_assignment(C)
    return math.fsum(float(C[r, c]) for r, c in zip(rows, cols))


def lsap_bruteforce(C):
    """The optimal total of C [P, n] by trying every injective map gt -> prediction (n <= 6, P <= 8; in general at most
    200 000 maps).  Only there to check that scipy's optimum is the optimum on matrices with ties."""
    import itertools
    P, n = C.shape
    assert n <= P and math.perm(P, n) <= 200000, (P, n)
    return min(math.fsum(float(C[p, j]) for j, p in enumerate(ps)) for ps in itertools.permutations(range(P), n))


def min_gap_ulps(C):
    """The smallest gap between two entries of one row or one column of C, in float32 ulps of the largest finite |C|
    (0 if two are equal, inf if no row or column has two entries)."""
    fin = np.abs(C[np.isfinite(C)])
    u = ulp32(fin.max())
    best = np.inf
    for M in (C, C.T):
        if M.shape[1] > 1:
            with np.errstate(invalid="ignore"):
                d = np.diff(np.sort(M, axis=1), axis=1)
            best = min(best, float(np.nanmin(d)))
    return best / u


def second_best_margin(C):
    """How much worse than the optimum the best assignment is that differs from scipy's in at least one pair: each chosen
    pair is forbidden in turn and the problem solved again.  Zero means the optimum is not unique."""
    rows, cols = linear_sum_assignment(C)
    base = math.fsum(float(C[r, c]) for r, c in zip(rows, cols))
    best = np.inf
    for r, c in zip(rows, cols):
        C2 = C.copy()
        C2[r, c] = np.inf
        try:
            r2, c2 = linear_sum_assignment(C2)
        except ValueError:
            continue
        best = min(best, math.fsum(float(C2[a, b]) for a, b in zip(r2, c2)) - base)
    return best


def tie_bound(C, n):
    """8 * n * ulp32(max finite |C|): an entry of the device's matrix differs from the oracle's by at most 4 ulps (logf of the
    two confidence terms, 1 ulp each as HIP documents, and the two float32 additions behind them), so an assignment that
    is optimal for the device's matrix is within 2 * n * 4 ulps of optimal for the oracle's."""
    return 8.0 * n * ulp32(np.abs(C[np.isfinite(C)]).max())


def conf_from_logits(z):
    return (R.sigmoid_f32(z) + EPS).astype(np.float32)


# ------------------------------------------------------------------------------------------- mbx_match: tie-free inputs
MATCH_SEED = 20240              # first seed of every draw below; a draw that misses its precondition takes the next one
GAP_ULPS = 8.0
BOX_SHAPE = np.array([0.0, 0.03, 0.2, 0.25])


def random_image(P, n, seed):
    rng = np.random.RandomState(seed)
    dec = rng.uniform(0, 1, (P, 4)).astype(np.float32)
    conf = conf_from_logits(rng.randn(P) * 2 - 1)
    gt = rng.uniform(0, 1, (n, 4)).astype(np.float32)
    return dec, conf, gt


def _ladder_image(P, n, seed):
    """Uniform draws cannot keep P entries of a column 8 ulps apart once P is in the hundreds (the float32 grid under max|C|
    has 2^24 points and a column wants them pairwise distinct with room), so beyond that the image is built: predictions are
    one box shape at P positions x on a jittered ladder in [0.25, 0.75], their confidences fall as x grows, and the gt boxes
    are the same shape at n jittered ladder positions in [0, 0.15].  Every gt then ranks the predictions alike (heavy
    contention, long augmenting paths), consecutive entries of a column differ by at least 4000 * 0.1 * (step / 2) and the
    predictions are handed out in a random order, so the matched ones lie anywhere in [0, P)."""
    rng = np.random.RandomState(seed)
    x = 0.25 + (np.arange(P) + 0.5 + rng.uniform(-0.25, 0.25, P)) * (0.5 / P)
    logit = np.sort(rng.uniform(-3, 3, P))[::-1]
    y = (np.arange(n) + 0.5 + rng.uniform(-0.25, 0.25, n)) * (0.15 / max(n, 1))
    perm, permg = rng.permutation(P), rng.permutation(n)
    dec = (x[perm, None] + BOX_SHAPE).astype(np.float32)
    gt = (y[permg, None] + BOX_SHAPE).astype(np.float32)
    return dec, conf_from_logits(logit[perm]), gt.reshape(n, 4)


def tie_free_image(P, n, alpha, seed):
    """(dec [P,4], conf [P], gt [n,4], seed used): every row and column of the cost matrix has its entries more than GAP_ULPS
    float32 ulps of max|C| apart -- the condition under which the assignment may be compared exactly with scipy's although
    the device's logf may differ from numpy's in the last bit."""
    make = random_image if P <= 65 else _ladder_image
    for s in range(seed, seed + 400):
        dec, conf, gt = make(P, n, s)
        if n == 0 or min_gap_ulps(costs(dec, conf, gt, n, alpha)) > GAP_ULPS:
            return dec, conf, gt, s
    raise AssertionError("no tie-free draw for P=%d n=%d in 400 seeds" % (P, n))


def match_lds_bytes(P, G):
    """The host's formula (loss.hip, match_lds_bytes): 36 bytes a prediction, 16 a gt, 16 of padding."""
    return 36 * P + 16 * G + 16


# (B, P, G).  Where the P values come from: 63/64/65 are either side of a wavefront; 1536/1537 is the host's switch from 256
# to 512 threads (P > 1536); 1812/1813 are the two sides of match_lds_bytes(P, 16) = 64 KiB, where the launch starts to ask
# for more dynamic LDS; 4221 is the largest P with match_lds_bytes(P, 100) <= 150 KiB (test_postproc_oracle_cpu re-derives
# all of them from match_lds_bytes).
MATCH_SHAPES = [(2, 1, 1), (3, 63, 63), (3, 64, 64), (3, 65, 64), (2, 128, 128), (3, 1536, 20), (3, 1537, 20),
                (2, 1812, 16), (2, 1813, 16), (2, 4221, 100)]
MATCH_TOO_BIG = (1, 4222, 100)


def match_launch_case(B, P, G, alpha=1000.0):
    """Image 0 has n = min(G, P), image 1 has n = 0, the rest a random n.  Returns dec [B,P,4], conf [B,P], gt [B,G,4], n [B]."""
    rng = np.random.RandomState(MATCH_SEED + 7 * P + G)
    n = rng.randint(1, min(G, P) + 1, B).astype(np.int32)
    n[0] = min(G, P)
    if B > 1:
        n[1] = 0
    dec, conf, gt = np.zeros((B, P, 4), np.float32), np.zeros((B, P), np.float32), np.zeros((B, G, 4), np.float32)
    for b in range(B):
        dec[b], conf[b], g, _ = tie_free_image(P, int(n[b]), alpha, MATCH_SEED + 1000 * b)
        gt[b, :n[b]] = g
    return dec, conf, gt, n


def cost_matrix_lastbit(dec, conf, gt, alpha, rng=None):
    """ref_numpy.cost_matrix restated (byte-identical with rng None: test_postproc_oracle_cpu), with log c and log(1 - c) of
    every prediction moved by -1, 0 or +1 float32 ulp at random: what a device logf that is right to 1 ulp may return.
    These two logarithms are the only place where the device's matrix can differ from the oracle's."""
    dec, conf, gt = np.asarray(dec, np.float32), np.asarray(conf, np.float32), np.asarray(gt, np.float32).reshape(-1, 4)
    lc = np.log(conf)
    v = np.float32(1.0) - conf
    v[v > 1.0] = 1.0
    v[v <= 0] = R.SMALL_EPSILON
    l1c = np.log(v)
    if rng is not None:
        for a in (lc, l1c):
            k = rng.randint(-1, 2, len(a))
            a[k < 0] = np.nextafter(a[k < 0], np.float32(-np.inf))
            a[k > 0] = np.nextafter(a[k > 0], np.float32(np.inf))
    half_alpha = np.float32(np.float32(alpha) / np.float32(2.0))
    C = np.zeros((len(dec), len(gt)), np.float64)
    for j in range(len(gt)):
        d = dec - gt[j]
        s = d * d
        nrm = np.sqrt(((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3])
        C[:, j] = (half_alpha * (nrm ** 2) - lc) + l1c
    return C


def robust_to_log_lastbit(dec, conf, gt, alpha, trials=32):
    """Does scipy choose the same assignment on `trials` matrices whose logarithms were moved in the last bit?"""
    base = linear_sum_assignment(cost_matrix_lastbit(dec, conf, gt, alpha))
    rng = np.random.RandomState(MATCH_SEED)
    for _ in range(trials):
        got = linear_sum_assignment(cost_matrix_lastbit(dec, conf, gt, alpha, rng))
        if not (np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])):
            return False
    return True


def contention_flat_image(P=646, n=100):
    """Predictions in the unit square, alpha = 1e-3, all gt boxes inside a 0.01 neighbourhood of one box: the location term
    (5e-4 |l - g|^2, differences of 1e-5 between the boxes) is below the float32 grid of a cost of a few units, so the entries
    of a row are EQUAL in float32 and the optimum is not unique.  This is a tie case (match_tie_cases), not a tie-free one."""
    rng = np.random.RandomState(MATCH_SEED)
    dec = rng.uniform(0, 1, (P, 4)).astype(np.float32)
    gt = (np.array([0.3, 0.35, 0.6, 0.7]) + rng.uniform(-0.005, 0.005, (n, 4))).astype(np.float32)
    return dec, conf_from_logits(rng.randn(P) * 2 - 1), gt


def match_contention_case(alpha, P=646, n=100):
    """All gt boxes jittered inside a 0.01 neighbourhood of one box, so every gt ranks the predictions alike.  alpha = 1000:
    predictions in the unit square.  alpha = 1e-3: the confidence term decides which predictions are wanted, the same ones
    by every gt; the predictions are spread over [-40, 40] so that the location term still clears the float32 grid (in the
    unit square it does not: contention_flat_image).  The 8-ulp gap of the launch cases cannot hold here -- the entries of a
    row differ by the jitter only -- so the precondition for equality with scipy is checked on its cause: scipy's choice
    does not move when the two logarithms of every prediction move in the last bit (robust_to_log_lastbit); re-drawn with
    the next seed until it holds.  Returns dec [1,P,4], conf [1,P], gt [1,n,4], n [1], the seed used."""
    for s in range(MATCH_SEED, MATCH_SEED + 50):
        rng = np.random.RandomState(s)
        if alpha >= 1.0:
            dec = rng.uniform(0, 1, (P, 4)).astype(np.float32)
            conf = conf_from_logits(rng.randn(P) * 2 - 1)
        else:
            dec = rng.uniform(-40, 40, (P, 4)).astype(np.float32)
            conf = conf_from_logits(np.linspace(-3, 3, P)[rng.permutation(P)])
        gt = (np.array([0.3, 0.35, 0.6, 0.7]) + rng.uniform(-0.005, 0.005, (n, 4))).astype(np.float32)
        if robust_to_log_lastbit(dec, conf, gt, alpha):
            return dec[None], conf[None], gt[None], np.array([n], np.int32), s
    raise AssertionError("no contention draw whose optimum survives a last-bit change of the logarithms")


def match_special_case(kind, P=40, n=5, alpha=1000.0):
    """One tie-free image (the 8-ulp gap holds on its finite entries) for the status and padding tests.  kind: "plain";
    "conf_one": a confidence of exactly 1 and one of 1.5 (the w <= 0 -> 1e-10 branch) on two predictions next to a gt, which take them;
    "far_one": prediction 11 at 1e20, whose squared distance overflows float32, so its costs are +inf (scipy accepts +inf
    entries); "far_all": every prediction there (scipy raises: infeasible).  Returns dec [P,4], conf [P], gt [n,4]."""
    for s in range(MATCH_SEED, MATCH_SEED + 400):
        dec, conf, gt = random_image(P, n, s)
        if kind == "conf_one":
            conf[3], conf[17] = 1.0, 1.5
            dec[3], dec[17] = gt[0] + np.float32(0.01), gt[1] - np.float32(0.01)
        elif kind == "far_one":
            dec[11] = 1e20
        elif kind == "far_all":
            dec[:] = 1e20
            return dec, conf, gt
        else:
            assert kind == "plain", kind
        if min_gap_ulps(costs(dec, conf, gt, n, alpha)) > GAP_ULPS:
            return dec, conf, gt
    raise AssertionError("no tie-free draw for %s" % kind)


# ------------------------------------------------------------------------------------------------ mbx_match: tie inputs
def match_tie_cases(priors_k5):
    """name -> (dec [P,4], conf [P], gt [n,4], alpha).  Every case has equal entries in its cost matrix."""
    rng = np.random.RandomState(MATCH_SEED)
    out = {}
    dec = rng.uniform(0, 1, (8, 4)).astype(np.float32)
    gt = rng.uniform(0, 1, (6, 4)).astype(np.float32)
    gt[4] = gt[1]
    out["twin_gt"] = (dec, conf_from_logits(rng.randn(8)), gt, 1000.0)
    # 8 identical predictions, boxes and confidence, close to all 3 gts and confident: the cheapest of 40 for each of them
    dec = rng.uniform(0, 1, (40, 4)).astype(np.float32)
    z = (rng.randn(40) - 2).astype(np.float32)
    gt = (np.array([0.4, 0.4, 0.6, 0.6]) + rng.uniform(-0.02, 0.02, (3, 4))).astype(np.float32)
    twins = np.array([3, 7, 12, 13, 21, 30, 38, 39])
    dec[twins], z[twins] = np.array([0.4, 0.4, 0.6, 0.6], np.float32), 3.0
    out["twin_predictions"] = (dec, conf_from_logits(z), gt, 1000.0)
    out["all_equal"] = (np.tile(np.array([[0.2, 0.3, 0.5, 0.7]], np.float32), (70, 1)), np.full(70, 0.25, np.float32) + EPS,
                        np.tile(np.array([[0.25, 0.25, 0.5, 0.75]], np.float32), (5, 1)), 1000.0)
    # start of training: the predictions are the priors, every logit equal, 4 boxes symmetric about the image centre
    # (each box is centred on a mirror axis of the prior grid, so a prior and its mirror image cost it the same)
    gt = np.array([[0.4375, 0.25, 0.5625, 0.375], [0.4375, 0.625, 0.5625, 0.75],
                   [0.25, 0.4375, 0.375, 0.5625], [0.625, 0.4375, 0.75, 0.5625]], np.float32)
    out["start_of_training"] = (np.asarray(priors_k5, np.float32), np.full(len(priors_k5), 0.5, np.float32) + EPS, gt, 1000.0)
    out["contention_flat"] = contention_flat_image() + (1e-3,)
    return out


def reduce_for_bruteforce(C):
    """The rows (predictions) an optimal assignment can need: for every gt its n cheapest, with everything tied with the
    n-th.  (A gt matched outside its n cheapest has one of them free and can move there at no loss.)"""
    P, n = C.shape
    rows = set()
    for j in range(n):
        cut = np.sort(C[:, j])[n - 1]
        rows.update(np.nonzero(C[:, j] <= cut)[0].tolist())
    return C[sorted(rows)]


# --------------------------------------------------------------------------------------------------- mbx_decode_conf
def sigmoid_ref(z, eps_add):
    """sigmoid(z) + eps_add in float64 on the float32 inputs, rounded once to float32."""
    z = np.asarray(z, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-z))
    return (s + float(np.float32(eps_add))).astype(np.float32)


# ------------------------------------------------------------------------------------------- mbx_decode_filter_topk
def make_meta(B, offsets=(0, 0), dims=(299, 299), flips=0, res=(0, 0, 1, 1), mtk=200, hw=None):
    """The per-patch columns as a dict of arrays; scalars and single rows are broadcast to B patches."""
    m = dict(offsets=np.broadcast_to(np.asarray(offsets, np.int32), (B, 2)).copy(),
             dims=np.broadcast_to(np.asarray(dims, np.int32), (B, 2)).copy(),
             flips=np.broadcast_to(np.asarray(flips, np.int32), (B,)).copy(),
             res=np.broadcast_to(np.asarray(res, np.float32), (B, 4)).copy(),
             mtk=np.broadcast_to(np.asarray(mtk, np.int32), (B,)).copy())
    m["hw"] = m["dims"].copy() if hw is None else np.broadcast_to(np.asarray(hw, np.int32), (B, 2)).copy()
    return m


def take_meta(meta, idx):
    return {k: v[idx].copy() for k, v in meta.items()}


def topk_expected(raw, conf, priors, meta, k_max):
    """The kernel's four outputs from ref_numpy.detect_postprocess with float32 restrictions:
    count = clamp(min(kept, max_to_keep), 0, k_max); slots at or past count are 0.0 / 0.0f / -1."""
    B = raw.shape[0]
    eb, es = np.zeros((B, k_max, 4), np.float64), np.zeros((B, k_max), np.float32)
    ei, ec = np.full((B, k_max), -1, np.int32), np.zeros((B,), np.int32)
    for b in range(B):
        limit = min(max(int(meta["mtk"][b]), 0), k_max)
        rb, rs, ridx = R.detect_postprocess(raw[b], conf[b], priors, meta["res"][b], limit, meta["offsets"][b],
                                            meta["dims"][b], meta["hw"][b], int(meta["flips"][b]))
        c = len(ridx)
        eb[b, :c], es[b, :c], ei[b, :c], ec[b] = rb, rs, ridx, c
    return eb, es, ei, ec


def topk_random_case(B, P, seed, mtk=200):
    """Random boxes around random priors; some decode outside [0, 1] (clipped) and the patches have different restrictions,
    so each of them drops a different share."""
    rng = np.random.RandomState(seed)
    xy = rng.uniform(0, 0.8, (P, 2))
    priors = np.concatenate([xy, xy + rng.uniform(0.02, 0.3, (P, 2))], 1).astype(np.float32)
    raw = (rng.randn(B, P, 4) * 0.05).astype(np.float32)
    conf = R.sigmoid_f32(rng.randn(B, P) * 2)
    res = np.array([[0, 0, 1, 1], [0.1, 0.1, 0.9, 0.9], [0, 0.1, 1, 0.9], [0.1, 0, 0.9, 1]], np.float32)[np.arange(B) % 4]
    return raw, conf, priors, make_meta(B, res=res, mtk=mtk, dims=(480, 640))


def _raw_for(target, prior):
    """A float32 raw with float32(raw + prior) bit-equal to target."""
    target, prior = np.float32(target), np.float32(prior)
    r = np.float32(target - prior)
    lo = hi = r
    for _ in range(4):
        for cand in (lo, hi):
            if np.float32(cand + prior) == target:
                return np.float32(cand)
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    raise AssertionError("no raw decodes to %r from prior %r" % (target, prior))


BOUNDARY_RES = np.array([0.1, 0.1, 0.9, 0.9], np.float32)
BOUNDARY_GROUPS = ("equal", "outside", "inside")


def topk_boundary_case():
    """Three patches of 9 predictions, restrictions (0.1, 0.1, 0.9, 0.9) as float32.  Patch 0: decoded corners bit-equal to a
    restriction (kept: the filter is strict); patch 1: one float32 ulp outside it (dropped); patch 2: one ulp inside (kept).
    In each patch predictions 0-3 have one corner there and the others well inside, prediction 4 has all four there, and
    5-8 are well inside.  Returns raw [3,9,4], conf [3,9], priors [9,4], meta, and the float32 targets [3,9,4]."""
    rng = np.random.RandomState(MATCH_SEED)
    P = 9
    # priors close to the restrictions: a raw offset below 1/16 lies on a finer float32 grid than 0.1 and 0.9, so every target
    # bit pattern can be reached
    priors = np.concatenate([rng.uniform(0.12, 0.14, (P, 2)), rng.uniform(0.86, 0.88, (P, 2))], 1).astype(np.float32)
    out_dir = np.array([-np.inf, -np.inf, np.inf, np.inf], np.float32)      # the side of each restriction that drops
    target = np.zeros((3, P, 4), np.float32)
    for g, name in enumerate(BOUNDARY_GROUPS):
        edge = {"equal": BOUNDARY_RES, "outside": np.nextafter(BOUNDARY_RES, out_dir),
                "inside": np.nextafter(BOUNDARY_RES, -out_dir)}[name]
        target[g] = priors + rng.uniform(-0.005, 0.005, (P, 4)).astype(np.float32)
        for k in range(4):
            target[g, k, k] = edge[k]
        target[g, 4] = edge
    raw = np.zeros((3, P, 4), np.float32)
    for idx in np.ndindex(3, P, 4):
        raw[idx] = _raw_for(target[idx], priors[idx[1:]])
    conf = R.sigmoid_f32(rng.randn(3, P))
    return raw, conf, priors, make_meta(3, res=BOUNDARY_RES, mtk=200), target


# ------------------------------------------------------------------------------------------------------------ mbx_nms
def nms_lds_bytes(k_max):
    """The host's formula (postproc.hip, mbx_nms): k_max bit rows of W 64-bit words and one row for the removed set."""
    W = (k_max + 63) // 64
    return (k_max * W + W) * 8


def nms_lds_crossing():
    """(largest k_max whose LDS fits 64 KiB, the next one): where mbx_nms starts to ask for more dynamic LDS."""
    k = max(k for k in range(1, 1025) if nms_lds_bytes(k) <= 65536)
    assert nms_lds_bytes(k + 1) > 65536
    return k, k + 1


NMS_THRESHOLDS = (0.0, 0.5, 1.0)
NMS_PATTERNS = ("chain", "identical", "disjoint", "clustered", "last_sweep")


def nms_boxes(pattern, K, seed=0):
    """K boxes [K,4] float64 in stored (score) order."""
    rng = np.random.RandomState(MATCH_SEED + seed)
    i = np.arange(K, dtype=np.float64)
    if pattern == "chain":          # unit squares 1/4 apart: IoU(i, i+1) = 0.6, IoU(i, i+2) = 1/3, all dyadic coordinates
        return np.stack([i * 0.25, 0 * i, i * 0.25 + 1.0, 0 * i + 1.0], 1)
    if pattern == "identical":
        return np.tile([[0.25, 0.125, 0.75, 0.5]], (K, 1))
    if pattern == "disjoint":
        return np.stack([2 * i, 0 * i, 2 * i + 1.0, 0 * i + 1.0], 1)
    if pattern == "clustered":
        c = rng.uniform(0.1, 0.7, (max(K // 12, 1), 2))[rng.randint(0, max(K // 12, 1), K)]
        xy, wh = c + rng.uniform(-0.03, 0.03, (K, 2)), rng.uniform(0.08, 0.2, (K, 2))
        return np.concatenate([xy, xy + wh], 1)
    if pattern == "last_sweep":     # all copies of box 0 up to the last 256-box sweep of the compaction, disjoint boxes in it:
        base = (K - 1) // 256 * 256  # the survivors other than box 0 are read in the last sweep and land in the first
        b = np.tile([[0.0, 2.0, 1.0, 3.0]], (K, 1))
        b[base:] = np.stack([2 * i, 0 * i, 2 * i + 1.0, 0 * i + 1.0], 1)[base:]
        return b
    raise KeyError(pattern)


def nms_greedy_vec(boxes, thr):
    """ref_numpy.nms_greedy with the inner loop over the kept boxes done as one numpy expression: the same float64
    operations in the same order on every pair, hence the same decisions (test_postproc_oracle_cpu checks it), at a cost
    that allows 1024 boxes of which all survive."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    keep = []
    for i in range(len(b)):
        if keep:
            k = b[keep]
            iw = np.minimum(k[:, 2], b[i, 2]) - np.maximum(k[:, 0], b[i, 0])
            ih = np.minimum(k[:, 3], b[i, 3]) - np.maximum(k[:, 1], b[i, 1])
            inter = np.where((iw > 0.0) & (ih > 0.0), iw * ih, 0.0)
            union = area[keep] + area[i] - inter
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = np.where(union > 0.0, inter / union, 0.0)
            if (iou > thr).any():
                continue
        keep.append(i)
    return np.array(keep, np.int64)


def nms_expected(boxes, scores, index, count, k_max, thr, greedy=nms_greedy_vec):
    """The buffers after mbx_nms: per row the survivors of boxes[:clamp(count, 0, k_max)] moved to the front, in order, and
    the new count.  Slots at or past the new count are not compared (the kernel leaves what was there)."""
    out = []
    for b in range(len(count)):
        K = min(max(int(count[b]), 0), k_max)
        keep = greedy(boxes[b, :K], thr)
        out.append((len(keep), boxes[b][keep], scores[b][keep], index[b][keep]))
    return out
