"""What the GPU tests of the loss entries share (test_gpu_loss_mined.py, test_gpu_loss_focal.py, test_gpu_match_extend.py):
the seeded inputs with a hand-made match, one call of the C ABI for each of the three entries, and the batch that goes
through MultiboxLoss.  A plain module: the fixtures are imported by name into the test modules that use them."""
import numpy as np
import pytest

from tests import mined_oracle as MO

ALPHA = 1000.0
SHAPES = [(3, 13, 13), (4, 70, 5), (4, 646, 13), (2, 3199, 100)]
SENTINEL = 7.0


def weights(alpha):
    return (1.0, 1.0) if alpha is None else (alpha, 1.0 - alpha)


@pytest.fixture(scope="module")
def gpu():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from multibox_amd import _lib
    return torch, _lib.lib()


def make_case(B, P, G, kind="plain", seed=0):
    """Seeded inputs with a hand-made match: image 0 has no positive, image 1 the most there can be (min(G, P): at
    (3, 13, 13) it has no negative at all), the others a random number.  `x` holds confidences in (0, 1) -- `kind` says
    which -- and `z` logits."""
    rng = np.random.RandomState(1000 * P + B + seed)
    n_pos = rng.randint(1, min(G, P) + 1, B)
    n_pos[0], n_pos[1] = 0, min(G, P)
    match = -np.ones((B, P), np.int32)
    for b in range(B):
        match[b, rng.permutation(P)[:n_pos[b]]] = rng.permutation(G)[:n_pos[b]]
    x = rng.uniform(0.01, 0.99, (B, P)).astype(np.float32)
    if kind == "quantised":                                   # 16 levels: long runs of equal keys
        x = (np.floor(x * 16) / 16).astype(np.float32)
    elif kind == "zeros":                                     # most entries +0.0 or -0.0: one run of equal keys, two bit patterns
        r = rng.uniform(size=(B, P))
        x = np.where(r < 0.4, np.float32(0.0), np.where(r < 0.8, np.float32(-0.0), x)).astype(np.float32)
    return dict(B=B, P=P, G=G, n_pos=n_pos, match=match, x=x, z=(rng.randn(B, P) * 2 - 1).astype(np.float32),
                dec=rng.uniform(0, 1, (B, P, 4)).astype(np.float32), gt=rng.uniform(0, 1, (B, G, 4)).astype(np.float32))


def call(gpu, c, conf_in, is_logit, entry="focal", gamma=2.0, alpha=0.25, neg_per_pos=0, min_neg=0, rows=None,
         grad_scale=1.0, ws_short=0, prefill=None, w=None):
    """One call of the C ABI on images `rows` of case c -> (status, dict of numpy outputs).  entry: "focal", "mined" or
    "plain"; `w` overrides the weights that `alpha` stands for; the workspace is passed as ws_short bytes less than asked."""
    torch, l = gpu
    rows = slice(None) if rows is None else rows
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).cuda()
    dec, x, gt, match = dev(c["dec"]), dev(conf_in), dev(c["gt"]), dev(c["match"])
    B, P, G = match.shape[0], c["P"], c["G"]
    fill = (lambda *s, dt=torch.float32: torch.full(s, prefill, dtype=dt, device="cuda")) if prefill is not None else \
        (lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device="cuda"))
    loss2, dl, dz, n_neg = fill(2), fill(B, P, 4), fill(B, P), fill(B, dt=torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    head = (dec.data_ptr(), x.data_ptr(), int(is_logit), gt.data_ptr(), match.data_ptr(), ALPHA, grad_scale, B, P, G,
            loss2.data_ptr(), dl.data_ptr(), dz.data_ptr())
    if entry == "focal":
        w_pos, w_neg = weights(alpha) if w is None else w
        ws = torch.empty((l.mbx_loss_focal_workspace_bytes(B, P),), dtype=torch.uint8, device="cuda")
        st = l.mbx_loss_fwd_bwd_focal(*head, gamma, w_pos, w_neg, neg_per_pos, min_neg, n_neg.data_ptr(), ws.data_ptr(),
                                      ws.numel() - ws_short, s)
    elif entry == "mined":
        ws = torch.empty((l.mbx_loss_mined_workspace_bytes(B, P),), dtype=torch.uint8, device="cuda")
        st = l.mbx_loss_fwd_bwd_mined(*head, neg_per_pos, min_neg, n_neg.data_ptr(), ws.data_ptr(), ws.numel() - ws_short, s)
    else:
        assert entry == "plain"
        ws = torch.empty((l.mbx_loss_workspace_bytes(B),), dtype=torch.uint8, device="cuda")
        st = l.mbx_loss_fwd_bwd(*head, ws.data_ptr(), ws.numel() - ws_short, s)
    torch.cuda.synchronize()
    return st, dict(loss2=loss2.cpu().numpy(), dl=dl.cpu().numpy(), dz=dz.cpu().numpy(), n_neg=n_neg.cpu().numpy())


def cut_splits_a_run(c, mask):
    """Images in which negatives with bit-equal keys lie on both sides of the cut."""
    key = MO.score_order_key(c["x"])
    hit = []
    for b in range(c["B"]):
        neg = c["match"][b] < 0
        if np.intersect1d(key[b][neg & mask[b]], key[b][neg & ~mask[b]]).size:
            hit.append(b)
    return hit


@pytest.fixture(scope="module")
def batch():
    """Raw network outputs and ground truth for MultiboxLoss at P = 646, B = 4 (image 1 without boxes)."""
    from multibox_amd import priors as PR
    priors = np.array(PR.generate_priors([1, 2, 3, 1 / 2., 1 / 3.]), np.float32)
    rng = np.random.RandomState(5)
    B, P, G = 4, priors.shape[0], 13
    raw = (rng.randn(B, P, 4) * 0.05).astype(np.float32)
    logits = (rng.randn(B, P) * 2 - 2).astype(np.float32)
    n = np.array([G, 0, 3, 7], np.int32)
    gt = np.zeros((B, G, 4), np.float32)
    for b in range(B):
        xy = rng.uniform(0, .7, (n[b], 2)); wh = rng.uniform(.05, .3, (n[b], 2))
        gt[b, :n[b], :2] = xy; gt[b, :n[b], 2:] = xy + wh
    return dict(priors=priors, raw=raw, logits=logits, gt=gt, n=n, B=B, P=P, G=G)


def _forward_backward(torch, ml, batch):
    """MultiboxLoss.forward_backward on the batch -> [loss2, d_locs, d_logits] as numpy; the match must have succeeded."""
    out = ml.forward_backward(torch.from_numpy(batch["raw"]).cuda(), torch.from_numpy(batch["logits"]).cuda(),
                              torch.from_numpy(batch["gt"]).cuda(), torch.from_numpy(batch["n"]).cuda())
    torch.cuda.synchronize()
    assert int(ml.status.max()) == 0
    return [t.cpu().numpy() for t in out]
