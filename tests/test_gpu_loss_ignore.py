"""GPU: mbx_loss_fwd_bwd_ignore (the loss with the ignore band) against mbx_loss_fwd_bwd_quality and tests/ignore_oracle.py,
then the band through MultiboxLoss and the Trainer.

The C ABI is driven with the hand-made `match` of tests.loc_oracle.make_loc_case (tests/loss_cases.py's, with boxes that mean
something to an IoU) and a subset of its free priors set to -2 by hand.  Bars:
  * with no -2 in `match` every output is mbx_loss_fwd_bwd_quality's, byte for byte;
  * with -2 present the kept priors are gathered on the GPU into one compact problem per image and run through
    mbx_loss_fwd_bwd_quality: d_logits and d_raw_locs of the kept priors, n_neg and the count in q_stats are its bytes; the
    ignored priors have all-zero gradients, sign bit included;
  * loss2 and the sum in q_stats follow the float64 oracle at tests/test_gpu_loss_quality.py's bars for the same quantities
    (confidence loss rtol 1e-5, location loss rtol 1e-6, the sum of q rtol 1e-12): the same terms in another lane order."""
import numpy as np
import pytest

from tests import atss_cases as AC
from tests import atss_oracle as AO
from tests import extend_oracle as EO
from tests import ignore_oracle as IO
from tests import loc_oracle as LO
from tests import mined_oracle as MO
from tests import quality_oracle as QO
from tests.loss_cases import ALPHA, SENTINEL, SHAPES, _forward_backward, batch, gpu  # noqa: F401
from tests.test_gpu_loss_loc import TYPE

pytestmark = pytest.mark.gpu

OUTPUTS = ("loss2", "dl", "dz", "n_neg", "q_stats")


def launch(gpu, entry, dec, x, gt, match, is_logit, quality, loc_type, gamma, w, neg_per_pos, min_neg, grad_scale, stats=True,
           prefill=None, ws_short=0):
    """One call of `entry` ("ignore" or "quality") on CUDA tensors -> (status, dict of numpy outputs)."""
    torch, l = gpu
    B, P = match.shape
    G = gt.shape[1]
    fill = (lambda *s, dt=torch.float32: torch.full(s, prefill, dtype=dt, device="cuda")) if prefill is not None else \
        (lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda"))
    loss2, dl, dz, n_neg, qs = fill(2), fill(B, P, 4), fill(B, P), fill(B, dt=torch.int32), fill(B, 2, dt=torch.float64)
    ws = torch.empty((getattr(l, "mbx_loss_%s_workspace_bytes" % entry)(B, P),), dtype=torch.uint8, device="cuda")
    st = getattr(l, "mbx_loss_fwd_bwd_" + entry)(
        dec.data_ptr(), x.data_ptr(), int(is_logit), gt.data_ptr(), match.data_ptr(), ALPHA, grad_scale, B, P, G,
        loss2.data_ptr(), dl.data_ptr(), dz.data_ptr(), TYPE.get(loc_type, loc_type), LO.BETA, QO.QUALITY.get(quality, quality),
        gamma, w[0], w[1], neg_per_pos, min_neg, n_neg.data_ptr(), qs.data_ptr() if stats else None, ws.data_ptr(),
        ws.numel() - ws_short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, dict(loss2=loss2.cpu().numpy(), dl=dl.cpu().numpy(), dz=dz.cpu().numpy(), n_neg=n_neg.cpu().numpy(),
                    q_stats=qs.cpu().numpy())


def both(gpu, c, match, x, is_logit, quality, loc_type, gamma=2.0, w=(1.0, 0.75), neg_per_pos=0, min_neg=0, grad_scale=1.0):
    """mbx_loss_fwd_bwd_ignore on the whole case with `match`, and mbx_loss_fwd_bwd_quality on every image's kept priors,
    gathered on the GPU and scattered back into zeros -> (ignore's outputs, the compact runs' outputs, kept [B,P])."""
    torch, _ = gpu
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dec, xs, gt, m = dev(c["dec"]), dev(x), dev(c["gt"]), dev(match)
    stats = quality != "none"
    args = (is_logit, quality, loc_type, gamma, w, neg_per_pos, min_neg, grad_scale, stats)
    st, out = launch(gpu, "ignore", dec, xs, gt, m, *args)
    assert st == 0
    B, P = match.shape
    ref = dict(dl=np.zeros((B, P, 4), np.float32), dz=np.zeros((B, P), np.float32), n_neg=np.zeros(B, np.int32),
               q_stats=np.zeros((B, 2)))
    kept = m != -2
    for b in range(B):
        k = torch.nonzero(kept[b]).reshape(-1)
        if k.numel() == 0:
            continue
        st, one = launch(gpu, "quality", dec[b:b + 1, k].contiguous(), xs[b:b + 1, k].contiguous(), gt[b:b + 1],
                         m[b:b + 1, k].contiguous(), *args)
        assert st == 0
        kk = k.cpu().numpy()
        ref["dl"][b, kk], ref["dz"][b, kk] = one["dl"][0], one["dz"][0]
        ref["n_neg"][b], ref["q_stats"][b] = one["n_neg"][0], one["q_stats"][0]
    return out, ref, kept.cpu().numpy()


def check_against_compaction(out, ref, kept, oracle, quality, what=""):
    """The bars of the module docstring; every figure is printed before it is asserted."""
    rel_c = abs(float(out["loss2"][1]) - oracle["conf_loss"]) / max(abs(oracle["conf_loss"]), 1e-300)
    rel_l = abs(float(out["loss2"][0]) - oracle["loc_loss"]) / max(abs(oracle["loc_loss"]), 1e-300)
    print("%s ignored %s n_neg %s; conf_loss %r oracle %r rel %.3g; loc_loss %r oracle %r rel %.3g" % (
        what, (~kept).sum(1).tolist(), out["n_neg"].tolist(), out["loss2"][1], oracle["conf_loss"], rel_c, out["loss2"][0],
        oracle["loc_loss"], rel_l))
    assert out["dz"].tobytes() == ref["dz"].tobytes() and out["dl"].tobytes() == ref["dl"].tobytes()
    assert not out["dz"].view(np.uint32)[~kept].any() and not out["dl"].view(np.uint32)[~kept].any()      # +0: no sign bit
    assert np.array_equal(out["n_neg"], ref["n_neg"]) and np.array_equal(out["n_neg"], oracle["n_neg"])
    assert np.isclose(out["loss2"][1], oracle["conf_loss"], rtol=1e-5, atol=0)
    assert np.isclose(out["loss2"][0], oracle["loc_loss"], rtol=1e-6, atol=0)
    if quality != "none":
        q_rel = np.abs(out["q_stats"][:, 0] - oracle["q_stats"][:, 0]) / np.maximum(np.abs(oracle["q_stats"][:, 0]), 1e-300)
        print("   q sums %s oracle %s worst rel %.3g" % (out["q_stats"][:, 0].tolist(), oracle["q_stats"][:, 0].tolist(), q_rel.max()))
        assert out["q_stats"][:, 1].tobytes() == ref["q_stats"][:, 1].tobytes()
        assert np.array_equal(out["q_stats"][:, 1], oracle["q_stats"][:, 1])
        assert np.allclose(out["q_stats"][:, 0], oracle["q_stats"][:, 0], rtol=1e-12, atol=0)


def oracle_for(c, match, x, is_logit, quality, loc_type, gamma=2.0, w=(1.0, 0.75), neg_per_pos=0, min_neg=0, **_):
    return IO.loss(None if quality == "none" else quality, loc_type, c["dec"], x, is_logit, c["gt"], match, ALPHA, gamma, w[0],
                   w[1], neg_per_pos, min_neg)


@pytest.fixture(scope="module")
def cases():
    return {s: LO.make_loc_case(*s) for s in SHAPES}


def with_ignored(c, every=3):
    """c's match with every `every`-th free prior (counted over the batch) set to -2 by hand."""
    match = c["match"].copy()
    free = np.nonzero(match.reshape(-1) == -1)[0]
    match.reshape(-1)[free[::every]] = -2
    return match


# ------------------------------------------------------------------------- 1. no -2: mbx_loss_fwd_bwd_quality's bytes
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_without_an_ignored_prior_every_output_is_the_quality_entrys(gpu, cases, B, P, G, neg_per_pos):
    torch, _ = gpu
    c = cases[(B, P, G)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dec, z, gt, m = dev(c["dec"]), dev(c["z"]), dev(c["gt"]), dev(c["match"])
    assert not (c["match"] == -2).any()
    for i, (quality, loc_type) in enumerate([(q, t) for q in ("none", "qfl", "varifocal") for t in ("l2", "giou")]):
        args = (1, quality, loc_type, 2.0, (0.25, 0.75), neg_per_pos, 2 if neg_per_pos else 0, (1.0, 0.25, -2.0)[i % 3],
                quality != "none")
        st_q, ref = launch(gpu, "quality", dec, z, gt, m, *args, prefill=SENTINEL)
        st_i, out = launch(gpu, "ignore", dec, z, gt, m, *args, prefill=SENTINEL)
        assert st_q == 0 and st_i == 0
        for k in OUTPUTS:
            assert out[k].tobytes() == ref[k].tobytes(), (k, quality, loc_type)
        assert not np.any(out["dz"] == SENTINEL) and not np.any(out["n_neg"] == int(SENTINEL))


# ---------------------------------------------------------------------------------- 2. with -2: the compact problem
@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("quality,loc_type,neg_per_pos,min_neg,is_logit,grad_scale", [
    ("none", "l2", 0, 0, 1, 1.0), ("none", "giou", 3, 0, 0, -1.0), ("qfl", "giou", 0, 0, 1, -1.0), ("qfl", "l2", 3, 2, 1, 0.25),
    ("varifocal", "ciou", 3, 0, 1, -1.0), ("varifocal", "l2", 0, 0, 0, 1.0)])
def test_with_ignored_priors_the_rest_is_the_compact_problem(gpu, cases, B, P, G, quality, loc_type, neg_per_pos, min_neg,
                                                             is_logit, grad_scale):
    c = cases[(B, P, G)]
    match = with_ignored(c)
    assert (match == -2).sum() >= 1
    x = c["z"] if is_logit else c["x"]
    kw = dict(quality=quality, loc_type=loc_type, neg_per_pos=neg_per_pos, min_neg=min_neg)
    out, ref, kept = both(gpu, c, match, x, is_logit, grad_scale=grad_scale, **kw)
    oracle = oracle_for(c, match, x, is_logit, **kw)
    assert np.array_equal(kept, oracle["kept"])
    oracle = dict(oracle, conf_loss=oracle["conf_loss"], loc_loss=oracle["loc_loss"])
    check_against_compaction(out, ref, kept, oracle, quality, "P=%d %s %s neg_per_pos=%d:" % (P, quality, loc_type, neg_per_pos))
    n_pos = (match >= 0).sum(1)
    if not neg_per_pos:
        assert np.array_equal(out["n_neg"], P - n_pos - (match == -2).sum(1))
    else:
        assert np.array_equal(out["n_neg"], np.minimum(np.maximum(min_neg, neg_per_pos * n_pos), (kept & (match < 0)).sum(1)))
    # the gradients against the oracle too, at the quality tests' bars: the compact runs are held to it, not only to themselves
    want = grad_scale * oracle["d_conf_in"]
    atol = 1e-6 * min(1.0, abs(grad_scale))
    assert np.allclose(out["dz"], want, rtol=1e-4, atol=atol)


# ------------------------------------------------------------------------------------------------ 3. the mining budget
@pytest.mark.parametrize("B,P,G", SHAPES[1:])                 # (3, 13, 13): image 1 has no negative, the others too few to mine
@pytest.mark.parametrize("quality", ["none", "qfl"])
def test_mining_budget(gpu, cases, B, P, G, quality):
    c = cases[(B, P, G)]
    z = c["z"]
    mask, K = MO.select(z, c["match"], 3, 0)
    b = B - 1                                                 # an image with a random number of positives
    assert 0 < K[b] < (c["match"][b] < 0).sum() - K[b]
    # every prior mining would have selected is ignored: the budget stays and moves on to the next K
    match = c["match"].copy()
    match[b, mask[b] & (match[b] < 0)] = -2
    kw = dict(quality=quality, loc_type="giou", neg_per_pos=3)
    out, ref, kept = both(gpu, c, match, z, 1, **kw)
    check_against_compaction(out, ref, kept, oracle_for(c, match, z, 1, **kw), quality, "selected ones ignored:")
    assert out["n_neg"][b] == K[b] and not out["dz"][b][match[b] == -2].any()
    assert ((out["dz"][b] != 0) & (match[b] == -1)).sum() == K[b]
    # min_neg above what is left: every remaining negative, and no more
    match = with_ignored(c, 2)
    kw = dict(quality=quality, loc_type="giou", neg_per_pos=3, min_neg=P)
    out, ref, kept = both(gpu, c, match, z, 1, **kw)
    check_against_compaction(out, ref, kept, oracle_for(c, match, z, 1, **kw), quality, "min_neg = P:")
    assert np.array_equal(out["n_neg"], (match == -1).sum(1)) and (out["n_neg"] < P - (match >= 0).sum(1))[1:].all()
    # every free prior ignored: K = 0, the positives alone
    match = np.where(c["match"] == -1, -2, c["match"]).astype(np.int32)
    kw = dict(quality=quality, loc_type="giou", neg_per_pos=3, min_neg=5)
    out, ref, kept = both(gpu, c, match, z, 1, **kw)
    check_against_compaction(out, ref, kept, oracle_for(c, match, z, 1, **kw), quality, "all free ignored:")
    assert not out["n_neg"].any() and not out["dz"][match < 0].any() and out["dz"][match >= 0].all()
    out, _, _ = both(gpu, c, match, z, 1, quality=quality, loc_type="giou")     # and unmined: no negative is left
    assert not out["n_neg"].any() and not out["dz"][match < 0].any()


@pytest.mark.parametrize("B,P,G", SHAPES)
@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_other_negative_values_are_negatives(gpu, cases, B, P, G, neg_per_pos):
    torch, _ = gpu
    c = cases[(B, P, G)]
    base = with_ignored(c)
    other = base.copy()
    free = np.nonzero(other.reshape(-1) == -1)[0]
    other.reshape(-1)[free[::2]] = -3
    other.reshape(-1)[free[1::5]] = -77
    assert (other == -3).any() and (other == -77).any() and (other == -2).any()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dec, z, gt = dev(c["dec"]), dev(c["z"]), dev(c["gt"])
    args = (1, "qfl", "giou", 2.0, (1.0, 1.0), neg_per_pos, 0, -1.0)
    st_a, a = launch(gpu, "ignore", dec, z, gt, dev(base), *args)
    st_b, b = launch(gpu, "ignore", dec, z, gt, dev(other), *args)
    assert st_a == 0 and st_b == 0
    for k in OUTPUTS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["dz"][other == -3].all() if not neg_per_pos else a["dz"][other == -3].any()


# ------------------------------------------------------------------------------------------------ 4. refusals, repeats
@pytest.mark.parametrize("kw,status", [
    (dict(quality=-1), -1), (dict(quality=3), -1), (dict(quality="qfl", gamma=0.5), -1), (dict(gamma=float("nan")), -1),
    (dict(quality="none"), -1),                               # q_stats with MBX_QUALITY_NONE
    (dict(loc_type=5), -1), (dict(w=(-1.0, 1.0)), -1), (dict(neg_per_pos=-1), -1), (dict(neg_per_pos=0, min_neg=1), -1),
    (dict(ws_short=1), -4), (dict(quality=3, ws_short=1), -1)])
def test_bad_arguments_are_refused_and_nothing_is_written(gpu, cases, kw, status):
    torch, _ = gpu
    c = cases[(4, 70, 5)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = dict(dict(quality="qfl", loc_type="giou", gamma=2.0, w=(1.0, 1.0), neg_per_pos=0, min_neg=0), **kw)
    st, out = launch(gpu, "ignore", dev(c["dec"]), dev(c["z"]), dev(c["gt"]), dev(with_ignored(c)), 1, kw["quality"],
                     kw["loc_type"], kw["gamma"], kw["w"], kw["neg_per_pos"], kw["min_neg"], 1.0, prefill=SENTINEL,
                     ws_short=kw.get("ws_short", 0))
    assert st == status
    for k in ("loss2", "dl", "dz", "q_stats"):
        assert np.all(out[k] == SENTINEL), k
    assert np.all(out["n_neg"] == int(SENTINEL))


@pytest.mark.parametrize("neg_per_pos", [0, 3])
def test_an_image_depends_on_its_own_row_only_and_calls_repeat(gpu, cases, neg_per_pos):
    torch, _ = gpu
    c = cases[(4, 646, 13)]
    match = with_ignored(c)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = (1, "varifocal", "giou", 2.0, (1.0, 0.75), neg_per_pos, 0, 0.25)
    run = lambda rows: launch(gpu, "ignore", dev(c["dec"][rows]), dev(c["z"][rows]), dev(c["gt"][rows]), dev(match[rows]), *args)
    st, whole = run(slice(None))
    st2, again = run(slice(None))
    assert st == 0 and st2 == 0
    for k in OUTPUTS:
        assert whole[k].tobytes() == again[k].tobytes(), k
    rows = [3, 2, 1, 0, 2]
    st, moved = run(rows)
    assert st == 0
    for k in ("dl", "dz", "n_neg", "q_stats"):
        for i, b in enumerate(rows):
            assert moved[k][i].tobytes() == whole[k][b].tobytes(), (k, b)
    # NULL gradients, n_neg and q_stats: loss2 alone, the same bytes
    l = gpu[1]
    loss2 = torch.zeros(2, device="cuda")
    ws = torch.empty((l.mbx_loss_ignore_workspace_bytes(4, 646),), dtype=torch.uint8, device="cuda")
    t = [dev(c["dec"]), dev(c["z"]), dev(c["gt"]), dev(match)]
    st = l.mbx_loss_fwd_bwd_ignore(t[0].data_ptr(), t[1].data_ptr(), 1, t[2].data_ptr(), t[3].data_ptr(), ALPHA, 0.25, 4, 646, 13,
                                   loss2.data_ptr(), None, None, TYPE["giou"], 0.0, 2, 2.0, 1.0, 0.75, neg_per_pos, 0, None, None,
                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0 and loss2.cpu().numpy().tobytes() == whole["loss2"].tobytes()


# ------------------------------------------------------------------------------------------------ 5. through MultiboxLoss
def _chained(torch, ml, batch, rule):
    """The oracles chained on the step's own bipartite match: (match, n_ignored) after `rule` and the band at 0.3."""
    from multibox_amd import loss as L
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bip, st = L.match_boxes(ml.decoded, ml.conf, dev(batch["gt"]), dev(batch["n"]), ml.alpha)
    torch.cuda.synchronize()
    assert int(st.max()) == 0
    bip, status = bip.cpu().numpy(), np.zeros(batch["B"], np.int32)
    assert np.array_equal((bip >= 0).sum(1), batch["n"])
    if rule == "threshold":
        ext, extra = EO.extend(batch["priors"], batch["gt"], batch["n"], status, bip, 0.5)
    else:
        ext, extra, _ = AO.atss(batch["priors"], AC.LEVELS_299, batch["gt"], batch["n"], status, bip, 9)
    return IO.ignore(batch["priors"], 0, batch["gt"], batch["n"], status, ext, 0.3) + (extra,)


@pytest.mark.parametrize("rule", ["threshold", "atss"])
def test_multibox_loss_composes_matching_band_and_mining(gpu, batch, rule):
    torch, _ = gpu
    from multibox_amd import loss as L
    kw = dict(match_iou_threshold=0.5) if rule == "threshold" else dict(atss_topk=9, prior_levels=AC.LEVELS_299)
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, ignore_iou_threshold=0.3, neg_per_pos=3, **kw)
    assert ml.entry == "mbx_loss_fwd_bwd_ignore"
    loss2, dl, dz = _forward_backward(torch, ml, batch)
    match, n_ignored = ml.match.cpu().numpy(), ml.n_ignored.cpu().numpy()
    want, want_n, extra = _chained(torch, ml, batch, rule)
    print(rule, "added", extra, "ignored", n_ignored, "oracle", want_n)
    assert want_n.sum() >= 1 and want_n[1] == 0               # the batch ignores something; image 1 has no box
    assert match.tobytes() == want.tobytes() and np.array_equal(n_ignored, want_n)
    assert np.array_equal(ml.n_extra.cpu().numpy() if rule == "threshold" else ml.n_atss.cpu().numpy(), extra)
    ref = IO.loss(None, "l2", ml.decoded.cpu().numpy(), batch["logits"], 1, batch["gt"], match, ALPHA, 0.0, 1.0, 1.0, 3, 0)
    n_neg = ml.n_neg.cpu().numpy()
    assert np.array_equal(n_neg, ref["n_neg"])
    assert np.array_equal(n_neg, np.minimum(3 * (match >= 0).sum(1), (match == -1).sum(1)))
    assert not dz.view(np.uint32)[match == -2].any() and not dl.view(np.uint32)[match < 0].any()
    assert np.allclose(dz, ref["d_conf_in"], rtol=1e-4, atol=1e-6)
    top = float(np.abs(ref["dl"]).max())
    assert np.allclose(dl, ref["dl"].astype(np.float32), rtol=1e-6, atol=1e-6 * top)
    assert np.isclose(loss2[1], ref["conf_loss"], rtol=1e-5, atol=0) and np.isclose(loss2[0], ref["loc_loss"], rtol=1e-6, atol=0)


def test_multibox_loss_by_the_predictions_overlap_and_without_the_switch(gpu, batch):
    torch, _ = gpu
    from multibox_amd import loss as L
    ml = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, ignore_iou_threshold=0.3, ignore_source="prediction",
                        quality_target="qfl", loc_loss="giou")
    loss2, dl, dz = _forward_backward(torch, ml, batch)
    match, dec = ml.match.cpu().numpy(), ml.decoded.cpu().numpy()
    bip = np.where(match >= 0, match, -1).astype(np.int32)
    want, want_n = IO.ignore(dec, 1, batch["gt"], batch["n"], np.zeros(batch["B"], np.int32), bip, 0.3)
    assert want_n.sum() >= 1 and match.tobytes() == want.tobytes() and np.array_equal(ml.n_ignored.cpu().numpy(), want_n)
    ref = IO.loss("qfl", "giou", dec, batch["logits"], 1, batch["gt"], match, ALPHA, 2.0, 1.0, 1.0)
    assert np.allclose(dz, ref["d_conf_in"], rtol=1e-4, atol=1e-6) and not dz.view(np.uint32)[match == -2].any()
    assert np.isclose(loss2[1], ref["conf_loss"], rtol=1e-5, atol=0)
    assert np.array_equal(ml.q_stats.cpu().numpy()[:, 1], ref["q_stats"][:, 1])
    # the switch off: the entries and the bytes of the call as it always was
    for kw in (dict(), dict(neg_per_pos=3, min_neg=2), dict(quality_target="qfl", loc_loss="giou")):
        old = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, **kw)
        new = L.MultiboxLoss(batch["priors"], batch["B"], batch["G"], ALPHA, ignore_iou_threshold=None, ignore_source="prior", **kw)
        assert new.ignore is None and new.n_ignored is None and new.entry == old.entry and new.entry != "mbx_loss_fwd_bwd_ignore"
        assert len(new.entry_args) == len(old.entry_args) and new.ws.numel() == old.ws.numel()
        for x, y in zip(_forward_backward(torch, old, batch), _forward_backward(torch, new, batch)):
            assert x.tobytes() == y.tobytes()
        assert not (new.match.cpu().numpy() == -2).any()


# ---------------------------------------------------------------------------------------------------- 6. through the Trainer
def test_trainer_step_with_the_band_graph_equals_eager(gpu):
    torch, _ = gpu
    from multibox_amd.engine import Net
    from multibox_amd.trainer import Trainer
    from multibox_amd import priors as PR, loss as L
    priors = np.array(PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.]), np.float32)
    gen = torch.Generator().manual_seed(3)
    images = torch.rand(2, 299, 299, 3, generator=gen) * 2 - 1
    rng = np.random.RandomState(1)
    n_gt = np.array([3, 0], np.int32)
    gt = np.zeros((2, 13, 4), np.float32)
    xy = rng.uniform(0, .7, (3, 2)); wh = rng.uniform(.05, .3, (3, 2))
    gt[0, :3, :2] = xy; gt[0, :3, 2:] = xy + wh
    res = []
    for use_graph in (True, False):
        net = Net(batch=2, input_size=299, k=5, mode="train", seed=5)
        tr = Trainer(net, priors, max_num_bboxes=13, use_graph=use_graph, ignore_iou_threshold=0.3, neg_per_pos=3)
        assert tr.loss.entry == "mbx_loss_fwd_bwd_ignore" and tr.loss.ignore == (0.3, 0)
        tr.set_batch(images.cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(n_gt).cuda())
        tr.step()
        torch.cuda.synchronize()
        assert int(tr.match_status().max()) == 0
        match, n_ignored = tr.loss.match.cpu().numpy(), tr.loss.n_ignored.cpu().numpy()
        bip, st = L.match_boxes(tr.loss.decoded, tr.loss.conf, tr.gt, tr.n_gt, tr.loss.alpha)
        torch.cuda.synchronize()
        bip = bip.cpu().numpy()
        assert int(st.max()) == 0 and (bip >= 0).sum(1).tolist() == [3, 0]
        want, want_n = IO.ignore(priors, 0, gt, n_gt, np.zeros(2, np.int32), bip, 0.3)
        print("ignored per image", n_ignored)
        assert match.tobytes() == want.tobytes() and np.array_equal(n_ignored, want_n)
        assert n_ignored[0] > 0 and n_ignored[1] == 0
        assert tr.ignored_per_image() == float(n_ignored.mean())
        d_logits = net.d_logits.reshape(2, -1).cpu().numpy()
        assert not d_logits.view(np.uint32)[match == -2].any()
        assert np.array_equal(tr.loss.n_neg.cpu().numpy(), np.minimum(3 * (match >= 0).sum(1), (match == -1).sum(1)))
        res.append((tr.loss.loss2.cpu().numpy(), match, n_ignored, d_logits))
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all()
    # without the key: nothing to report, and the entry the parent picked (a second trainer on the last net; never stepped)
    tr = Trainer(net, priors, max_num_bboxes=13, use_graph=False)
    assert tr.ignored_per_image() is None and tr.loss.n_ignored is None
    assert tr.loss.entry == "mbx_loss_fwd_bwd" and tr.loss.entry_args == ()
    assert Trainer(net, priors, max_num_bboxes=13, use_graph=False, neg_per_pos=3).loss.entry == "mbx_loss_fwd_bwd_mined"
