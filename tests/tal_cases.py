"""The inputs that tests/test_tal_cpu.py (the oracle's properties) and tests/test_gpu_match_tal.py (the kernel against the
oracle) share, and the oracle's result on each, computed once per process.  A plain module; nobody writes to its arrays.

A case is (B, P, G, topk, alpha, beta).  Priors, boxes and the partial pre-match are built as tests/atss_cases.py builds
them: random priors (or the project's real ones), boxes that are jittered copies of random priors, a random subset of the
priors already matched to distinct boxes.  Image 0 has no box, the last image min(G, P) of them.  On top of that the
predictions: `decoded` = the priors plus a uniform jitter of +-0.02 per image, `conf` float32 uniform in (0.01, 0.99)."""
import functools

import numpy as np

from tests import tal_oracle as TO
from tests.atss_cases import real_priors

LATTICE = 64

#        name           B  P     G    topk alpha beta priors   lattice  wide
CASES = {
    "p13":         (3, 13, 13, 3, 1.0, 6, "random", 0, False),          # fewer priors than one wavefront
    "p70":         (4, 70, 5, 4, 1.0, 6, "random", 0, False),           # P no multiple of 64
    "p70_lattice": (4, 70, 5, 4, 1.0, 6, "random", LATTICE, False),     # equal t on both sides of the cut
    "p70_top1":    (4, 70, 5, 1, 1.0, 6, "random", 0, False),
    "p70_all":     (4, 70, 5, 70, 1.0, 6, "random", 0, False),          # every candidate is selected, no round runs
    "p70_sqrt":    (4, 70, 5, 4, 0.5, 6, "random", 0, False),           # the square-root branch
    "p70_iou":     (4, 70, 5, 4, 0.0, 1, "random", 0, False),           # t = u
    "p646":        (4, 646, 13, 13, 1.0, 6, "299", 0, False),           # the real priors at 299 px
    "p646_deep":   (2, 646, 13, 300, 1.0, 6, "299", 0, True),          # a lane hands out more than it keeps: it scans again
    "p3199":       (2, 3199, 100, 13, 1.0, 6, "512", 0, False),         # the real priors at 512 px, boxes in a row on each wavefront
}


@functools.lru_cache(maxsize=None)
def make_case(name):
    B, P, G, topk, alpha, beta, kind, lattice, wide = CASES[name]
    rng = np.random.RandomState(1000 * P + B + lattice)
    c = rng.uniform(0.1, 0.9, (P, 2)); half = rng.uniform(0.05, 0.4, (P, 2)) / 2
    if lattice:
        # centres and half sizes on the lattice: corners, areas and intersections are exact; every three consecutive
        # priors share one centre, as the priors of one cell do, so they are inside the same boxes
        c, half = np.round(c * lattice) / lattice, np.maximum(np.round(half * lattice), 1) / lattice
        c = c[3 * (np.arange(P) // 3)]
    priors = np.concatenate([c - half, c + half], 1).astype(np.float32) if kind == "random" else real_priors(kind)
    assert priors.shape == (P, 4)
    n = rng.randint(1, min(G, P) + 1, B)
    n[0], n[-1] = 0, min(G, P)
    gt = np.zeros((B, G, 4), np.float32)
    match = -np.ones((B, P), np.int32)
    for b in range(B):
        gt[b, :n[b]] = priors[rng.randint(0, P, n[b])] + rng.uniform(-0.02, 0.02, (n[b], 4)).astype(np.float32)
        k = max(rng.randint(0, n[b] + 1), int(b == B - 1))     # the fullest image has at least one prior matched
        match[b, rng.permutation(P)[:k]] = rng.permutation(n[b])[:k]
    if wide:
        # box 0 of the last image covers nearly everything: some 600 candidates of which topk are taken, ten priors a lane
        gt[-1, 0] = [0.02, 0.02, 0.98, 0.98]
    decoded = (priors[None] + rng.uniform(-0.02, 0.02, (B, P, 4))).astype(np.float32)
    conf = rng.uniform(0.01, 0.99, (B, P)).astype(np.float32)
    if lattice:
        # everything on the lattice, the scores from three exact values, and every three consecutive priors predict one
        # box with one score: equal t, on both sides of the cut
        gt = (np.round(gt * lattice) / lattice).astype(np.float32)
        decoded = (np.round(decoded * lattice) / lattice).astype(np.float32)
        conf = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), (B, P))
        group = 3 * (np.arange(P) // 3)
        decoded, conf = decoded[:, group], conf[:, group]
    case = dict(name=name, B=B, P=P, G=G, topk=topk, alpha=alpha, beta=beta, priors=priors,
                decoded=np.ascontiguousarray(decoded), conf=np.ascontiguousarray(conf), gt=gt, n=n.astype(np.int32),
                status=np.zeros(B, np.int32), match=match)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(match, n_extra, thr) of the oracle on the case."""
    c = make_case(name)
    out = TO.tal(c["priors"], c["decoded"], c["conf"], c["gt"], c["n"], c["status"], c["match"], c["topk"], c["alpha"],
                 c["beta"])
    for a in out:
        a.setflags(write=False)
    return out
