"""Every form of the batch-norm backward against the float64 formula (tests/exact_ref.py bn_backward_ref), on statistics
chosen to hurt: the three-launch form (mask from the stored activation / recomputed from y / through a channel map), the
one-launch form (uncapped, 192 workgroups, mapped), mbx_bn_bwd_apply_rows on a table built here, the pooled pair, and the fused
tail of a data gradient.

Regimes, in blocks of 8 channels inside ONE launch (block b of shape number s gets REGIMES[(b + s) % 6]):
  benign     y ~ N(0.3, 1.5), mean / rstd its statistics
  offset     y ~ N(8, 0.25): mean / std = 32 -- about the largest ratio that still leaves several distinct bf16 levels
  constant   y = one value per channel, mean = that value, rstd = 1 / sqrt(eps), |beta| >= 0.05
  dead       beta = -100: with relu every gradient is masked -- dy must be exactly 0 and dbeta unchanged
  sparse     the gradient is non-zero in rows 0 and M - 1 only
  arbitrary  mean / rstd unrelated to y (they are INPUTS of these entry points)

Mask ambiguity is removed, not tolerated: where |(y - mean) rstd + beta| < 1e-4 in float64 (or y == thr for the threshold
form) da is set to 0, so g = 0 under either decision and the element is still compared; such elements are at most 0.1 % of
the tensor (asserted; expected ~1e-4 of the benign channels: unit-normal density 0.4 x a window of 2e-4).  Where da is itself
an OUTPUT of the launch under test (fused tail) or gathered on the fly (pooled pair), the same is reached by moving y off the
kink / zeroing the pool gradients routed to those elements.

Tolerance, derived and not tuned: |dy - ref| <= 2^-8 |ref| + A.  2^-8 |ref| is half a bf16 ulp -- the rounding of the output
format.  A = 1e-5 max|ref| (per channel: the sums are per channel) covers float32 summation order: on the CPU the float32
restatement of the formula stays within 2.6e-7 max|ref| of float64 under sequential, pairwise and 256-row-blocked summation
and for the rows form rstd (sum g y - mean sum g), benign and offset, M = 1001 .. 78400; A is ~40x that, for atomic arrival
order.  Each test recomputes the restatement's error on its own data and asserts it below A / 8.
dbeta: |dbeta - ref| <= 1e-6 sum|g|.
"""
import functools

import pytest

from tests import bn_bwd_paths as P
from tests import exact_ref as E

pytestmark = pytest.mark.gpu

REGIMES = ["benign", "offset", "constant", "dead", "sparse", "arbitrary"]
EPS = 1e-3
WINDOW = 1e-4
A_REL = 1e-5
SHAPES = E.BN_ROW_SHAPES
POOLED_SHAPES = [(7, 11, 13, 24), (2, 35, 35, 96), (64, 17, 17, 160)]       # N, H, W, C with N H W = M of SHAPES
# (geometry, tile_config, max_workgroups, split): b17upcap, b35_3x3, b17_1x7 of FUSED_BWD_CASES (tests/test_gpu_conv.py)
FUSED = {
    "b17upcap": ((16, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)), 34, 20, (192, 192)),
    "b35_3x3": ((20, 35, 35, 48, 64, 3, 3, 1, (1, 1, 1, 1)), 97, 0, (48,)),
    "b17_1x7": ((40, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), 98, 0, (128,)),
}


@pytest.fixture(scope="module")
def T():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()
    return torch


def _bf(t):
    return E.bf16_rne(t.double())


@functools.lru_cache(maxsize=None)
def layer(M, Cc, si, seed=0):
    """y (bf16-exact float64), float32 mean / rstd / beta / thr, and the regime of every 8-channel block."""
    import torch
    gen = torch.Generator().manual_seed(M * 131 + Cc + 7919 * seed)
    y = torch.zeros((M, Cc), dtype=torch.float64)
    mean, rstd, beta = torch.zeros(Cc), torch.zeros(Cc), torch.zeros(Cc)
    regs = []
    for b in range(Cc // 8):
        reg = REGIMES[(b + si) % len(REGIMES)]
        regs.append(reg)
        sl = slice(8 * b, 8 * b + 8)
        if reg == "offset":
            yb = _bf(torch.randn(M, 8, generator=gen) * 0.25 + 8.0)
        elif reg == "constant":
            yb = _bf(((torch.arange(8) - 3.0) * 0.75 + 0.125).expand(M, 8))
        else:
            yb = _bf(torch.randn(M, 8, generator=gen) * 1.5 + 0.3)
        y[:, sl] = yb
        bt = torch.randn(8, generator=gen) * 0.3
        if reg == "constant":
            mean[sl], rstd[sl] = yb[0].float(), float(EPS ** -0.5)
            bt = torch.where(bt < 0, -1.0, 1.0) * bt.abs().clamp(min=0.05)
        elif reg == "arbitrary":
            mean[sl], rstd[sl] = torch.randn(8, generator=gen), torch.rand(8, generator=gen) * 1.7 + 0.3
        else:
            y32 = yb.float()
            mean[sl], rstd[sl] = y32.mean(0), torch.rsqrt(y32.var(0, unbiased=False) + EPS)
        if reg == "dead":
            bt = torch.full((8,), -100.0)
        beta[sl] = bt
    thr = (mean.double() - beta.double() / rstd.double()).float()
    return dict(y=y, mean=mean, rstd=rstd, beta=beta, thr=thr, regs=regs)


def ambiguous(L):
    pre = (L["y"] - L["mean"].double()) * L["rstd"].double() + L["beta"].double()
    return (pre.abs() < WINDOW) | (L["y"] == L["thr"].double())


@functools.lru_cache(maxsize=None)
def gradient(M, Cc, si):
    """da (bf16-exact) for layer(M, Cc, si): dense N(0, 1), rows 0 and M - 1 only in the sparse blocks, 0 on the kink."""
    import torch
    L = layer(M, Cc, si)
    gen = torch.Generator().manual_seed(M * 17 + Cc)
    da = _bf(torch.randn(M, Cc, generator=gen))
    for b, reg in enumerate(L["regs"]):
        if reg == "sparse" and M > 2:
            da[1:M - 1, 8 * b:8 * b + 8] = 0
    amb = ambiguous(L)
    assert float(amb.double().mean()) <= 1e-3
    da[amb] = 0
    return da


def reference(L, da, relu, dbeta_in):
    """float64 reference; with relu the three mask forms must give the same g on this data (the kink has been cleared)."""
    import torch
    M = da.shape[0]
    if not relu:
        return E.bn_backward_ref(da, L["y"], L["mean"], L["rstd"], M, None, dbeta_in) + (da.double(),)
    m = E.mask_from_y(L["y"], L["mean"], L["rstd"], L["beta"])
    act = _bf(torch.relu((L["y"] - L["mean"].double()) * L["rstd"].double() + L["beta"].double()))
    g = da.double() * m
    assert torch.equal(g, da.double() * E.mask_from_threshold(L["y"], L["thr"]))
    assert torch.equal(g, da.double() * E.mask_from_activation(act))
    return E.bn_backward_ref(da, L["y"], L["mean"], L["rstd"], M, m, dbeta_in) + (g,)


def float32_restatement_error(L, g, dy_ref):
    """max |float32 evaluation of the formula - float64| per channel (torch's float32 sums)."""
    g32, y32 = g.float(), L["y"].float()
    M = g.shape[0]
    xh = (y32 - L["mean"]) * L["rstd"]
    dy32 = L["rstd"] * (g32 - g32.sum(0) / M - xh * ((g32 * xh).sum(0) / M))
    return (dy32.double() - dy_ref).abs().max(0).values


def check(torch, label, L, dy, dbeta, dy_ref, dbeta_ref, g, dbeta_in, relu):
    chan_max = dy_ref.abs().max(0).values
    A = A_REL * chan_max
    spread = float32_restatement_error(L, g, dy_ref)
    assert bool((spread <= A / 8).all()), "%s: the float32 restatement itself is %.3g max|ref| from float64" % (
        label, float((spread / (chan_max + 1e-300)).max()))
    err = (dy - dy_ref).abs()
    over = err - (dy_ref.abs() * 2.0 ** -8 + A)
    derr = (dbeta - dbeta_ref).abs()
    dbound = 1e-6 * g.abs().sum(0)
    for b, reg in enumerate(L["regs"]):
        sl = slice(8 * b, 8 * b + 8)
        rel = float((torch.clamp(err[:, sl] - dy_ref[:, sl].abs() * 2.0 ** -8, min=0) / (chan_max[sl] + 1e-300)).max())
        print("%s block %d %-9s: dy err beyond half an ulp %.3g max|ref| (A = 1e-5), float32 restatement %.3g, dbeta err %.3g of sum|g|" % (
            label, b, reg, rel, float((spread[sl] / (chan_max[sl] + 1e-300)).max()),
            float((derr[sl] / (g[:, sl].abs().sum(0) + 1e-300)).max())))
    for b, reg in enumerate(L["regs"]):
        sl = slice(8 * b, 8 * b + 8)
        assert bool((over[:, sl] <= 0).all()), "%s block %d (%s): %d elements out of tolerance, worst %.3g beyond the bound, max|ref| %.3g" % (
            label, b, reg, int((over[:, sl] > 0).sum()), float(over[:, sl].max()), float(chan_max[sl].max()))
        assert bool((derr[sl] <= dbound[sl]).all()), "%s block %d (%s): dbeta err %.3g, bound %.3g" % (
            label, b, reg, float(derr[sl].max()), float(dbound[sl].min()))
        if reg == "dead" and relu:
            assert float(dy[:, sl].abs().max()) == 0 and torch.equal(dbeta[sl], dbeta_in[sl]), "%s block %d: dead channels" % (label, b)


def _dbeta_in(torch, Cc):
    return (torch.arange(Cc) % 5).double() * 0.25


@pytest.mark.parametrize("path", P.PLAIN_PATHS)
@pytest.mark.parametrize("si,shape", list(enumerate(SHAPES)), ids=["M%d_C%d" % s for s in SHAPES])
def test_bn_backward_against_float64(T, path, si, shape):
    torch = T
    M, Cc = shape
    if not P.path_accepts(path, M, Cc, 1, True):
        assert path.endswith("mapped") and Cc < 16 or path == "onepass_192", "%s refuses M %d C %d" % (path, M, Cc)
        return
    L, da = layer(M, Cc, si), gradient(M, Cc, si)
    dbeta_in = _dbeta_in(torch, Cc)
    dy_ref, dbeta_ref, g = reference(L, da, 1, dbeta_in)
    act = _bf(torch.relu((L["y"] - L["mean"].double()) * L["rstd"].double() + L["beta"].double()))
    dy, dbeta = P.run_plain(torch, path, da, L["y"], L["mean"], L["rstd"], L["beta"], 1, dbeta_in, act=act, thr=L["thr"])
    check(torch, "%s M %d C %d" % (path, M, Cc), L, dy, dbeta, dy_ref, dbeta_ref, g, dbeta_in, 1)


@pytest.mark.parametrize("si,shape", list(enumerate(POOLED_SHAPES, start=1)), ids=["%dx%dx%dx%d" % s for s in POOLED_SHAPES])
def test_bn_backward_pooled_against_float64(T, si, shape):
    """The pooled pair: the gradient is gathered from the pool's output gradient through mbx_maxpool_fwd's argmax.  The
    reference routes with float64 autograd through F.max_pool2d and rounds the sum of the (at most four) routed terms to bf16, which
    is what a stored activation gradient holds; pool gradients routed to an element on the kink are zeroed,
    and in the sparse blocks only the first and the last window carry a gradient."""
    torch = T
    N, H, W, Cc = shape
    M = N * H * W
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    L = layer(M, Cc, si)
    act = _bf(torch.relu((L["y"] - L["mean"].double()) * L["rstd"].double() + L["beta"].double())).reshape(N, H, W, Cc)
    gen = torch.Generator().manual_seed(M + Cc)
    gy = _bf(torch.randn(N, Ho, Wo, Cc, generator=gen))
    for b, reg in enumerate(L["regs"]):
        if reg == "sparse":
            keep = gy[:, :, :, 8 * b:8 * b + 8].clone()
            gy[:, :, :, 8 * b:8 * b + 8] = 0
            gy[0, 0, 0, 8 * b:8 * b + 8], gy[-1, -1, -1, 8 * b:8 * b + 8] = keep[0, 0, 0], keep[-1, -1, -1]
    _, idx = P.pooled_reference_da(torch, act, gy)                                  # idx [N, C, Ho, Wo] -> h * W + w
    amb = ambiguous(L).reshape(N, H * W, Cc).permute(0, 2, 1)                       # [N, C, H W]
    assert float(amb.double().mean()) <= 1e-3
    hit = torch.gather(amb, 2, idx.reshape(N, Cc, -1)).reshape(N, Cc, Ho, Wo).permute(0, 2, 3, 1)
    gy[hit] = 0
    da, _ = P.pooled_reference_da(torch, act, gy)
    da = _bf(da.reshape(M, Cc))                           # (the kernels round the gathered sum to bf16, as mbx_maxpool_bwd stores it)
    assert float(da[ambiguous(L)].abs().max() if bool(ambiguous(L).any()) else 0.0) == 0
    dbeta_in = _dbeta_in(torch, Cc)
    dy_ref, dbeta_ref, g = reference(L, da, 1, dbeta_in)
    arg = P.pooled_inputs(torch, act, gy.shape)
    dy, dbeta = P.run_pooled(torch, gy, arg, shape, L["y"], L["mean"], L["rstd"], L["beta"], 1, dbeta_in)
    check(torch, "pooled %dx%dx%dx%d" % shape, L, dy, dbeta, dy_ref, dbeta_ref, g, dbeta_in, 1)


@pytest.mark.parametrize("name", list(FUSED))
def test_bn_backward_fused_tail_against_float64(T, name):
    """The fused tail: da is whatever the data gradient of the same launch wrote (returned as stored; the existing test proves it
    bit-equal to the plain launch), so the kink is cleared by moving y (to y + 0.25 / rstd) instead of zeroing da, and the
    sparse blocks are dense.  Layers alternate relu / no relu as in FUSED_BWD_CASES."""
    torch = T
    g, cfg, cap, split = FUSED[name]
    N, H, W, Ci, Co, R, S, st, pads = g
    M = N * H * W
    gen = torch.Generator().manual_seed(12)
    dyX = _bf(torch.randn(N, H, W, Co, generator=gen))
    wd = _bf(torch.randn(Co, R, S, Ci, generator=gen) / (R * S * Ci) ** 0.5)
    layers = []
    for i, K in enumerate(split):
        L = dict(layer(M, K, i + 2, seed=i + 1))
        amb = ambiguous(L)
        assert float(amb.double().mean()) <= 1e-3
        y = L["y"].clone()
        y[amb] = _bf(y + 0.25 / L["rstd"].double())[amb]
        L["y"] = y
        assert not bool(ambiguous(L).any())
        L.update(K=K, relu=int(i % 2 == 0), dbeta_in=_dbeta_in(torch, K))
        layers.append(L)
    da, outs = P.run_fused_tail(torch, g, cfg, cap, dyX, wd, (0.17 if R * S == 1 else 0.0), layers)
    assert float(da.abs().max()) > 0
    c0 = 0
    for i, (L, (dy, dbeta)) in enumerate(zip(layers, outs)):
        K = L["K"]
        dy_ref, dbeta_ref, gg = reference(L, da[:, c0:c0 + K], L["relu"], L["dbeta_in"])
        check(torch, "fused %s layer %d" % (name, i), L, dy, dbeta, dy_ref, dbeta_ref, gg, L["dbeta_in"], L["relu"])
        c0 += K
