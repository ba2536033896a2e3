"""The host side of the engine -- batch-norm units, workspace offsets, launch descriptors and the two consumer-fusion
plans -- pinned against a record of what the engine built before its planners and unit bookkeeping were merged.

tests/golden/engine_plan.json holds, for Net(batch=2, 299, k=5, train, cpu) at full depth and at repeats (1, 1, 1), each
under the default environment and with the launch-rule thresholds lowered so that the rules fire at this batch: the
members of every batch-norm unit, the offsets the engine stores per convolution, the sizes of its workspaces, the number
of launches, every descriptor of tune_registry (addresses as null / non-null) and what both planners decide.  Names and
integers only; equality, no tolerance.  No GPU needed: the graph is built on the CPU and nothing is launched.
"""
import ctypes as C
import json
import os
import struct

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTHS = {"full": (10, 20, 9), "r111": (1, 1, 1)}
ENVS = {"default": {}, "rules": {"MBX_RESIDENT_MIN_IMAGES": "1", "MBX_DIRECTW_MIN_PIXELS": "1", "MBX_DIRECT3_MIN_PIXELS": "1"}}
OFFSETS = ("w_off", "beta_off", "stats_off", "stats16_off", "bn_ws_off", "dgrad_off")
SIZES = ("bn_ws", "stats16", "stats_scratch", "bwd_scratch", "Wd")


def _unit_members(op):
    return [op] if op.group is None else list(op.group.members)


def _desc_record(d):
    """(non-address fields as integers in field order -- rscale by its float32 bits --, names of the non-null address fields)"""
    vals, ptrs = [], []
    for name, ctype in d._fields_:
        v = getattr(d, name)
        if ctype is C.c_void_p:
            if v:
                ptrs.append(name)
        elif ctype is C.c_float:
            vals.append(struct.unpack("<I", struct.pack("<f", v))[0])
        else:
            vals.append(int(v))
    return vals, ptrs


def _plan_record(net, unit_attr, seg_attr):
    units, consumers = {}, {}
    for op in net.convs:
        u = getattr(op, unit_attr)
        if u is not None:
            members = list(getattr(u, "members", u))
            units[members[0].name] = [m.name for m in members]
        segs = getattr(op, seg_attr)
        if segs is not None:
            consumers[op.name] = [[c_rel, m.name, c_in, n] for c_rel, m, c_in, n in segs]
    return {"units": units, "consumers": consumers}


def record(Net, depth, env):
    """What the engine built for one configuration, as names and integers."""
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        net = Net(batch=2, input_size=299, k=5, mode="train", device="cpu", repeats=DEPTHS[depth])
        rec = {"units": [[m.name for m in _unit_members(op)] for op in net.convs
                         if op.kind == "bn" and _unit_members(op)[0] is op]}
        rec["offsets"] = {op.name: [int(getattr(op, a, -1)) for a in OFFSETS] for op in net.convs}
        rec["sizes"] = [int(getattr(net, a).numel()) for a in SIZES]
        rec["launches"] = [len(net.fwd_launches), len(net.bwd_launches)]
        rec["registry"] = [[key, what, *_desc_record(d)] for key, d, what in net.tune_registry]
        # both planners, run on the CPU-built graph (their gates want the option on and, for one, a cuda device: neither
        # planner touches the device)
        net.fuse_bwd = True
        net._plan_fused_bwd()
        rec["fused_bwd"] = _plan_record(net, "fb_unit", "fb_segments")
        net.bw_stats, net.dev = True, "cuda"
        net._plan_bw_stats()
        net.dev = "cpu"
        rec["bw_stats"] = _plan_record(net, "bw_unit", "bw_segments")
        return rec
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def pack(rec, descriptors):
    """A record as the golden file stores it: convolutions by their index in forward order instead of their names, a
    launch descriptor by its index in `descriptors` (the distinct ones; a descriptor that is not among them stays as it is)."""
    convs = list(rec["offsets"])
    ix = {n: i for i, n in enumerate(convs)}
    dix = {json.dumps(d): i for i, d in enumerate(descriptors)}

    def plan(p):
        assert all(lead == members[0] for lead, members in p["units"].items())
        return {"units": [[ix[m] for m in members] for members in p["units"].values()],
                "consumers": [[ix[x], [[c_rel, ix[m], c_in, n] for c_rel, m, c_in, n in segs]] for x, segs in p["consumers"].items()]}

    build = {"convs": convs, "units": [[ix[m] for m in u] for u in rec["units"]], "offsets": [rec["offsets"][n] for n in convs],
             "sizes": rec["sizes"], "launches": rec["launches"],
             "registry": [dix.get(json.dumps(d), d) for d in json.loads(json.dumps(rec["registry"]))]}
    return build, {"fused_bwd": plan(rec["fused_bwd"]), "bw_stats": plan(rec["bw_stats"])}


@pytest.fixture(scope="module")
def golden():
    """{"fields": names of the descriptor fields recorded, "descriptors": the distinct [key, what, field values, non-null
    address fields], depth: {"build": what pack() gives, the same under either environment, environment: both plans}}"""
    with open(os.path.join(HERE, "golden", "engine_plan.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def Net():
    import __graft_entry__ as g
    g.build()
    from multibox_amd.engine import Net
    return Net


def test_golden_is_not_trivial(golden):
    """The counts the record was taken for, at full depth: 131 units and 143 consumers, 40 of them multi-segment, from either
    planner; with the rules firing 129 and 141 for the fused backward (the stem's direct launches have no tail) and 9 and 11
    for the backward statistics (the whole-width and resident-image launches have no statistics epilogue either); 403
    descriptors, 199 forward and 204 data-gradient."""
    from multibox_amd import ops
    assert golden["fields"] == [n for n, t in ops.ConvDesc._fields_ if t is not C.c_void_p]
    for plan, env, counts in (("fused_bwd", "default", (131, 143)), ("fused_bwd", "rules", (129, 141)),
                              ("bw_stats", "default", (131, 143)), ("bw_stats", "rules", (9, 11))):
        p = golden["full"][env][plan]
        assert (len(p["units"]), len(p["consumers"])) == counts, (plan, env)
    for plan in ("fused_bwd", "bw_stats"):
        assert sum(len(segs) > 1 for _, segs in golden["full"]["default"][plan]["consumers"]) == 40
    whats = [golden["descriptors"][i][1] for i in golden["full"]["build"]["registry"]]
    assert (len(whats), whats.count("fwd"), whats.count("dgrad")) == (403, 199, 204)


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("depth", sorted(DEPTHS))
def test_engine_builds_the_recorded_plan(golden, Net, depth, env):
    want, want_plans = golden[depth]["build"], golden[depth][env]
    got, got_plans = pack(record(Net, depth, ENVS[env]), golden["descriptors"])
    assert sorted(got) == sorted(want)
    for part in ("convs", "units", "sizes", "launches"):
        assert got[part] == want[part], part
    for name, g, w in zip(want["convs"], got["offsets"], want["offsets"]):
        assert g == w, (name, OFFSETS)
    assert len(got["registry"]) == len(want["registry"])
    for i, (g, w) in enumerate(zip(got["registry"], want["registry"])):
        assert g == w, (i, golden["descriptors"][w][:2])
    for plan in ("fused_bwd", "bw_stats"):
        assert got_plans[plan] == want_plans[plan], plan


# ---------------------------------------------------------------------- the planner on a hand-made graph
class _Fake:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _view(buf, ch_off, Cc, ld=128):
    return _Fake(buf=buf, ch_off=ch_off, C=Cc, N=2, H=8, W=8, ld=ld, img_stride=8 * 8 * ld)


def _op(name, x, out, unit):
    """a fake 1x1 convolution with the attributes the planners read; `unit`: a batch-norm layer (a unit of one)"""
    from multibox_amd.engine import BnUnit
    op = _Fake(name=name, x=x, out=out, K=out.C, Cin=x.C, R=1, S=1, stride=1, rscale=0.0, kind="bn" if unit else "residual",
               trainable=True, need_dx=True, skip=None, unit=None, group=None, fused_pool=None)
    if unit:
        op.unit = BnUnit([op])
    return op


def _six_ops():
    """src --A--> a[0:40]   --X1 reads a[0:32]                  A and B are batch-norm layers, X1..X3 their consumers.
       src --B--> a[40:104] --X2 reads a[32:72]  (A | B)        X2's second segment starts at channel 8 of its input view:
                            --X3 reads a[72:104]                aligned to 8 channels, not to 32."""
    src, a, b, o = object(), object(), object(), object()
    A = _op("A", _view(src, 0, 8), _view(a, 0, 40), unit=True)
    B = _op("B", _view(src, 8, 8), _view(a, 40, 64), unit=True)
    X1 = _op("X1", _view(a, 0, 32), _view(o, 0, 8), unit=False)
    X2 = _op("X2", _view(a, 32, 40), _view(o, 8, 8), unit=False)
    X3 = _op("X3", _view(a, 72, 32), _view(o, 16, 8), unit=False)
    other = _op("other", _view(src, 16, 8), _view(b, 0, 8), unit=False)
    return [A, B, X1, X2, X3, other]


def _names(segs):
    return {X.name: [(c, m.name, ci, n) for c, m, ci, n in s] for X, s in segs.items()}


SIX_SEGMENTS = {"X1": [(0, "A", 0, 32)], "X2": [(0, "A", 32, 8), (8, "B", 0, 32)], "X3": [(0, "B", 32, 32)]}


def test_fixed_point_drops_a_unit_in_its_second_round():
    """B's consumer X3 is refused by the predicate, so unit B goes in round 1; X2 reads channels of BOTH units, so it stops
    being convertible in round 2, and unit A -- every consumer of which was convertible in round 1 -- goes with it."""
    from multibox_amd.engine import plan_consumer_fusion
    ops6 = _six_ops()
    A, B, X1, X2, X3, other = ops6
    asked = []

    def consumer_ok(X):
        asked.append(X.name)
        return X is not X3

    everything = dict(convs=ops6, fwd=ops6, unit_ok=lambda u: True, align=8)
    units, segs = plan_consumer_fusion(consumer_ok=consumer_ok, **everything)
    assert units == [] and segs == {}
    assert asked.count("X2") == 1 and asked.count("X1") == 2       # X2 passed round 1 and lost unit B before round 2
    # the same graph with every consumer accepted: both units, and X2's input tiled by two members
    units, segs = plan_consumer_fusion(consumer_ok=lambda X: True, **everything)
    assert [u.lead.name for u in units] == ["A", "B"] and _names(segs) == SIX_SEGMENTS
    # a segment that does not start on the alignment makes its consumer, and then everything, unconvertible
    units, segs = plan_consumer_fusion(consumer_ok=lambda X: True, **dict(everything, align=32))
    assert units == [] and segs == {}
    # a second reader of A's first channels as a SKIP tensor: X1 is no longer their only reader
    other.skip = _view(A.out.buf, 0, 32)
    units, segs = plan_consumer_fusion(consumer_ok=lambda X: True, **everything)
    assert units == [] and segs == {}
    # a unit the caller refuses is no unit: its consumers are not tiled by members
    other.skip = None
    units, segs = plan_consumer_fusion(consumer_ok=lambda X: True, **dict(everything, unit_ok=lambda u: u.lead is not B))
    assert units == [] and segs == {}


def test_the_two_planners_differ_in_their_alignment(Net):
    """The same six operations through the engine's two planners: the fused backward takes segments at multiples of 8
    channels (X2 converts), the backward statistics at multiples of 32 (X2 does not, and nothing is left)."""
    ops6 = _six_ops()
    A, B = ops6[:2]
    net = _Fake(convs=ops6, fwd=ops6, fuse_bwd=True, bw_stats=True, dev="cuda", n_cus=256)
    Net._plan_fused_bwd(net)
    assert [op.fb_unit for op in ops6] == [A.unit, B.unit, None, None, None, None]
    assert _names({op: op.fb_segments for op in ops6 if op.fb_segments is not None}) == SIX_SEGMENTS
    Net._plan_bw_stats(net)
    assert all(op.bw_unit is None and op.bw_segments is None for op in ops6)
