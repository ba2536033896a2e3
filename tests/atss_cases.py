"""The inputs that tests/test_atss_cpu.py (the oracle's properties) and tests/test_gpu_match_atss.py (the kernel against the
oracle) share, and the oracle's result on each, computed once per process.  A plain module; nobody writes to its arrays.

A case is (B, P, G, levels, topk).  Priors, boxes and the partial pre-match are built as `_case` of test_extend_cpu.py builds
them: random priors (or the project's real ones), boxes that are jittered copies of random priors, a random subset of the
priors already matched to distinct boxes.  Image 0 has no box, the last image min(G, P) of them."""
import functools

import numpy as np

from tests import atss_oracle as AO

LEVELS_299 = [0, 320, 500, 580, 625, 645, 646]                 # grids 8/6/4/3/2/1, 5 priors a cell
LEVELS_512 = [0, 1372, 2380, 2723, 2975, 3150, 3199]           # grids 14/12/7/6/5, 7 priors a cell, and the 7x7 single-prior head
LATTICE = 64

#        name           B  P     G    levels               topk  priors    lattice
CASES = {
    "p13":         (3, 13, 13, [0, 13], 3, "random", 0),
    "p70":         (4, 70, 5, [0, 40, 68, 70], 4, "random", 0),       # a level smaller than topk, P no multiple of 64
    "p70_lattice": (4, 70, 5, [0, 40, 68, 70], 4, "random", LATTICE),  # equal distances on both sides of the cut
    "p646":        (4, 646, 13, LEVELS_299, 9, "299", 0),              # the last level has one prior
    "p3199":       (2, 3199, 100, LEVELS_512, 9, "512", 0),
    "p70_top1":    (4, 70, 5, [0, 40, 68, 70], 1, "random", 0),
    "p70_all":     (4, 70, 5, [0, 40, 68, 70], 70, "random", 0),       # every prior is a candidate of every box
    # beyond the issue's list: ten priors a lane and 300 of 646 taken, so a lane hands out more pairs than it keeps from
    # one scan and the kernel has to scan the level again (and again)
    "p646_deep":   (2, 646, 13, [0, 646], 300, "299", 0),
}


def real_priors(kind):
    """The project's priors at 299 px (646) or 512 px (3 199), float32."""
    import __graft_entry__ as g
    g.build()                                                  # the priors come from the library (host code)
    from multibox_amd import priors as PR
    if kind == "299":
        return PR.priors_for_input_size([1, 2, 3, 1 / 2., 1 / 3.], 299).astype(np.float32)
    return PR.priors_for_input_size([1, 2, 3, 4, 1 / 2., 1 / 3., 1 / 4.], 512).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(name):
    B, P, G, levels, topk, kind, lattice = CASES[name]
    rng = np.random.RandomState(1000 * P + B + lattice)
    c = rng.uniform(0.1, 0.9, (P, 2)); half = rng.uniform(0.05, 0.4, (P, 2)) / 2
    if lattice:
        # centres and half sizes on the lattice, so corners, centres and squared distances are exact; on level 0 every
        # three consecutive priors share one centre, as the priors of one cell do: topk = 4 cuts through the second group
        c, half = np.round(c * lattice) / lattice, np.maximum(np.round(half * lattice), 1) / lattice
        top = levels[1]
        c[:top] = c[:top][3 * (np.arange(top) // 3)]
    priors = np.concatenate([c - half, c + half], 1).astype(np.float32) if kind == "random" else real_priors(kind)
    assert priors.shape == (P, 4)
    n = rng.randint(1, min(G, P) + 1, B)
    n[0], n[-1] = 0, min(G, P)
    gt = np.zeros((B, G, 4), np.float32)
    match = -np.ones((B, P), np.int32)
    for b in range(B):
        gt[b, :n[b]] = priors[rng.randint(0, P, n[b])] + rng.uniform(-0.02, 0.02, (n[b], 4)).astype(np.float32)
        k = rng.randint(0, n[b] + 1)
        match[b, rng.permutation(P)[:k]] = rng.permutation(n[b])[:k]
    if lattice:
        gt = (np.round(gt * lattice) / lattice).astype(np.float32)
    case = dict(name=name, B=B, P=P, G=G, levels=list(levels), topk=topk, priors=priors, gt=gt, n=n.astype(np.int32),
                status=np.zeros(B, np.int32), match=match)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(match, n_extra, thr) of the oracle on the case."""
    c = make_case(name)
    out = AO.atss(c["priors"], c["levels"], c["gt"], c["n"], c["status"], c["match"], c["topk"])
    for a in out:
        a.setflags(write=False)
    return out
