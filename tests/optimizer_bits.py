"""What pins the optimiser's exact bytes (tests/test_gpu_optimizer_bits.py): the cases, one SHA-256 per case, and the tool that
wrote tests/golden/optimizer_bits.json from the library of the commit BEFORE the optimiser kernels were given one element
body.  The digests are that commit's; they are never written from the code under test -- a digest that differs means a
rounding changed.

A case is two trainable steps and one frozen step from fixed inputs; its digest covers w, the slots, ema and the bf16 copy, and
where they exist the partial sums, the ratios and the clip block.  reg_loss is left out: float atomics, a free order.

  flat    every rule (RMSProp with momentum 0 and 0.9, test_optimizer_cpu.RULES) at the six sizes of test_gpu_optimizer.py --
          1, 3, 259, 259 one float off a 16-byte boundary, 100003, one grid stride of 16-byte groups plus 259 -- plain, with
          a clip scale of 1 and with one of 0.5
  trust   trust_oracle.CASES over three variables whose bounds fall off the chunk grid and off 4-element alignment, at
          offsets 0 and 1, plain and with the two scales: the norm pass, the ratios, the apply pass
  norm    mbx_grad_sqnorm over two ranges and mbx_clip_finalize, clipping and not

Writing the fixture (on the GPU, from a build of the parent commit):
  python -m tests.optimizer_bits --lib PATH/libmbx.so --parent COMMIT --write
"""
import argparse
import ctypes
import hashlib
import json
import os

import numpy as np

from tests import test_gpu_grad_clip as GC
from tests import test_gpu_optimizer as GO
from tests import test_gpu_trust as GT
from tests import test_optimizer_cpu as OC
from tests import trust_oracle as TO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_bits.json")
MODES = {"plain": None, "clip1": 1.0, "clip0.5": 0.5}
FLAT_RULES = [("rmsprop", dict(momentum=0.0)), ("rmsprop", dict(momentum=0.9))] + OC.RULES
N_SIZES = GO.N_SIZES
TRUST_LENGTHS = lambda CH: [259, CH + 6, 2 * CH + 1]          # bounds 259, CH + 265, 3 CH + 266: none on the grid, none a multiple of 4
TRUST_ADAPT = [1, 0, 1]
NORM_BOUNDS = {"clips": 3.0, "below": 1e9}
STEPS = (1, 1, 0)                                             # trainable, trainable, frozen


def rule_id(rule, kw):
    return rule + "".join(",%s=%g" % (k, float(v)) for k, v in sorted(kw.items()))


def groups():
    """{group: [case keys]}: one group is one parametrised test."""
    out = {}
    for rule, kw in FLAT_RULES:
        for mode in MODES:
            out["flat/%s/%s" % (rule_id(rule, kw), mode)] = ["flat/%s/%s/size%d" % (rule_id(rule, kw), mode, i) for i in range(N_SIZES)]
    for rule, kw in TO.CASES:
        out["trust/%s" % rule_id(rule, kw)] = ["trust/%s/%s/off%d" % (rule_id(rule, kw), mode, off) for mode in MODES for off in (0, 1)]
    out["norm"] = ["norm/%s" % k for k in NORM_BOUNDS]
    return out


def digest(torch, arrays):
    h = hashlib.sha256()
    for a in arrays:
        if isinstance(a, torch.Tensor):
            a = a.contiguous().view(torch.uint8).cpu().numpy()
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


_data = {}


def data(n, seed):
    if (n, seed) not in _data:
        _data[n, seed] = OC.kernel_data(n, seed)
    return _data[n, seed]


def flat_case(torch, l, rule, kw, mode, size):
    n, off = GC.sizes(l)[size]
    w, g, ema = data(n, 700 + size)
    clip = None if MODES[mode] is None else GO.clip_block(torch, MODES[mode])
    if rule == "rmsprop":
        st = GC.State(torch, w, g, off)                       # (ms 1, mom 0.25, ema w / 2)
        for trainable in STEPS:
            st.step(l, kw["momentum"], OC.KERNEL_WD, clip=clip, trainable=trainable)
    else:
        st = GO.State(torch, w, g, ema, off)
        for k, trainable in enumerate(STEPS):
            st.step(l, rule, kw, ctl=clip, clipped=int(clip is not None), trainable=trainable, calls=k)
    return digest(torch, st.tensors()[:5])


def trust_case(torch, l, rule, kw, mode, off):
    bounds = TO.bounds_of(TRUST_LENGTHS(int(l.mbx_trust_chunk_elems())))
    w, g, ema = data(int(bounds[-1]), 800)
    clip = None if MODES[mode] is None else GO.clip_block(torch, MODES[mode])
    c = dict(ctl=clip, clipped=int(clip is not None))
    st = GT.State(torch, l, w, g, ema, bounds, TRUST_ADAPT, off)
    for k, trainable in enumerate(STEPS):
        if trainable:
            st.norms(l, rule, kw, calls=k, **c)
        st.apply(l, rule, kw, calls=k, trainable=trainable, **c)
    return digest(torch, st.everything()[:5] + st.everything()[6:] + (() if clip is None else (clip,)))


def norm_case(torch, l, which):
    (ga, wa), (gb, _) = GC.data(100003, 11), GC.data(259, 12)
    ranges = [(GC.dev(torch, ga), GC.dev(torch, wa), GC.WD), (GC.dev(torch, gb, 1), None, 0.0)]
    clip, part, cnt, _ = GC.norm_block((torch, l), ranges, NORM_BOUNDS[which])
    return digest(torch, (part, clip, cnt))


def run(torch, l, key):
    """The digest of case `key` on library `l`."""
    kind, *rest = key.split("/")
    if kind == "norm":
        return norm_case(torch, l, rest[0])
    rule, kw = next(r for r in FLAT_RULES + TO.CASES if rule_id(*r) == rest[0])
    if kind == "flat":
        return flat_case(torch, l, rule, kw, rest[1], int(rest[2][4:]))
    return trust_case(torch, l, rule, kw, rest[1], int(rest[2][3:]))


def bind(path):
    """The library at `path` with the signatures of multibox_amd._lib."""
    import torch  # noqa: F401  (its HIP runtime first, as _lib.lib() does)
    from multibox_amd import _lib
    l = ctypes.CDLL(path)
    for name, (res, args) in _lib._SIGS.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = res, args
    return l


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", required=True, help="libmbx.so of the parent commit")
    ap.add_argument("--parent", required=True, help="that commit's hash")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    import torch
    l = bind(a.lib)
    keys = [k for ks in groups().values() for k in ks]
    runs = [{k: run(torch, l, k) for k in keys} for _ in range(2)]
    differ = [k for k in keys if runs[0][k] != runs[1][k]]
    if differ:
        raise SystemExit("two runs of one library differ, nothing written: %s" % differ)
    print("%d cases, two runs agree" % len(keys))
    if a.write:
        with open(GOLDEN, "w") as f:
            json.dump({"parent": a.parent, "digests": runs[0]}, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)


if __name__ == "__main__":
    main()
