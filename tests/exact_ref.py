"""Integer data and float64 / int64 references for the exact pixel-reduction tests -- plain numpy / torch-CPU, never the code
under test -- and the case tables the GPU tests and the CPU self-checks share.

Why integers: a bf16 x bf16 MFMA product of two small integers is an integer, and a float32 sum of integers is exact while
it stays below 2^24 -- so the result has the same bits for any tiling, split, atomic arrival order or workgroup count, and a
pixel that is dropped, counted twice or read from the wrong address changes it.  The generators make every value depend on
its position (n, h, w, c), so no two neighbours can be swapped unnoticed.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EXACT_LIMIT = 2 ** 24          # float32 holds every integer below it
BF16_INT_LIMIT = 256           # bf16 holds every integer up to it


# ------------------------------------------------------------------------------------------------ generators
def int_tensor(shape, coef=(3, 5, 2, 11), mod=7, off=3, salt=0):
    """int64 tensor of `shape` with value ((sum_i coef[i] index_i + sum_i index_i index_{i+1} + salt) mod `mod`) - `off`: small
    integers (exact in bf16) that depend on every index (no coefficient is a multiple of `mod`); the products keep a shift along
    two axes at once from cancelling.  coef is read from its END, so a [M, C] tensor uses the (w, c) coefficients."""
    assert len(shape) <= len(coef) and mod - 1 - off <= BF16_INT_LIMIT and off <= BF16_INT_LIMIT
    v = torch.full(tuple(shape), int(salt), dtype=torch.int64)
    cf = coef[len(coef) - len(shape):]
    assert all(k % mod for k in cf)
    idx = []
    for i, n in enumerate(shape):
        view = [1] * len(shape)
        view[i] = n
        idx.append(torch.arange(n, dtype=torch.int64).reshape(view))
    for i, k in enumerate(cf):
        v = v + k * idx[i]
        if i + 1 < len(idx):
            v = v + idx[i] * idx[i + 1]
    return v % mod - off


def _scramble(a, b):
    """A fixed pseudo-random 24-bit number from two small integers (tap positions and signs: a regular stride can cancel against
    the generators' period -- eight taps at stride 261 with alternating signs summed to 0 on every pixel of a mod-5 tensor)."""
    return ((a * 2654435761 + b * 40503 + 12345) * 2246822519 >> 13) & 0xffffff


def sparse_filter(Co, R, S, Ci, per_out=5):
    """[Co][R][S][Ci] int64 filter with entries in {-1, 0, 1}, at most `per_out` non-zeros per OUTPUT channel (forward use:
    |y| <= per_out * max|x|): the j-th one somewhere in the j-th part of the K range (r, s, c), so that every
    tap, every input channel group and every K slice of a split-K launch carries weight (k_coverage)."""
    w = torch.zeros(Co, R * S * Ci, dtype=torch.int64)
    n = R * S * Ci
    for k in range(Co):
        for j in range(per_out):
            h = _scramble(k, j)
            w[k, (j * n // per_out + h % max(1, n // per_out)) % n] = 1 if (h >> 20) & 1 else -1
    return w.reshape(Co, R, S, Ci)


def sparse_filter_dgrad(Co, R, S, Ci, per_in=8):
    """The same with at most `per_in` non-zeros per INPUT channel (data-gradient use: |dx| <= per_in * max|dy|)."""
    w = torch.zeros(Ci, Co * R * S, dtype=torch.int64)
    n = Co * R * S
    for c in range(Ci):
        for j in range(per_in):
            h = _scramble(c + 7777, j)
            w[c, (j * n // per_in + h % max(1, n // per_in)) % n] = 1 if (h >> 20) & 1 else -1
    return w.reshape(Ci, R, S, Co).permute(3, 1, 2, 0).contiguous()


def k_coverage(w, parts=8, transposed=False):
    """Smallest number of non-zeros in any of `parts` equal pieces of the reduction range -- (r, s, c) of a forward filter
    [Co][R][S][Ci], (r, s, k) of a data gradient's -- over all output channels: 0 means a piece of K no test value depends on."""
    flat = (w.permute(3, 1, 2, 0) if transposed else w).reshape(w.shape[3] if transposed else w.shape[0], -1)
    n = flat.shape[1]
    used = (flat != 0).sum(0)
    return min(int(used[i * n // parts:(i + 1) * n // parts].sum()) for i in range(parts))


def bf16_rne(a):
    """float64 array / tensor -> the nearest bf16 value (ties to even), returned as float64.  Directly from float64: a detour
    through float32 would round twice.  (Normal range only: no bf16 subnormals, no overflow -- nothing here is near either.)"""
    t = torch.as_tensor(a, dtype=torch.float64)
    m, e = np.frexp(t.numpy())                      # t = m * 2^e, 0.5 <= |m| < 1: eight significant bits = m * 256 rounded
    return torch.from_numpy(np.ldexp(np.rint(m * 256.0), e - 8))


def is_bf16_exact(t):
    return bool(torch.equal(t.double().to(torch.bfloat16).double(), t.double()))


# ------------------------------------------------------------------------------------------------ convolution references
def out_hw(H, W, R, S, stride, pads):
    return (H + pads[0] + pads[2] - R) // stride + 1, (W + pads[1] + pads[3] - S) // stride + 1


def _conv64(x, w, stride, pads):
    xt = F.pad(x.permute(0, 3, 1, 2), (pads[1], pads[3], pads[0], pads[2]))
    return F.conv2d(xt, w.permute(0, 3, 1, 2), stride=stride).permute(0, 2, 3, 1)


def conv_forward_ref(x, w, stride, pads):
    """x [N,H,W,C], w [K,R,S,C], pads (t, l, b, r) -> y [N,Ho,Wo,K], float64 (F.conv2d on the CPU)."""
    with torch.no_grad():
        return _conv64(x.double(), w.double(), stride, pads).contiguous()


def conv_dgrad_ref(w, dy, x_shape, stride, pads):
    """dx of sum(conv(x, w) * dy): float64 autograd through F.conv2d."""
    xr = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    (_conv64(xr, w.double(), stride, pads) * dy.double()).sum().backward()
    return xr.grad.contiguous()


def conv_wgrad_ref(x, dy, R, S, stride, pads):
    """(dw [K,R,S,C], db [K]) of sum(conv(x, w) * dy): float64 autograd through F.conv2d (linear in w: evaluated at w = 0)."""
    wr = torch.zeros(dy.shape[-1], R, S, x.shape[-1], dtype=torch.float64, requires_grad=True)
    (_conv64(x.double(), wr, stride, pads) * dy.double()).sum().backward()
    return wr.grad.contiguous(), dy.double().reshape(-1, dy.shape[-1]).sum(0)


# ------------------------------------------------------------------------------------------------ batch-norm backward reference
def bn_backward_ref(da, y, mean, rstd, M, mask=None, dbeta_in=0.0):
    """float64: g = mask ? da : 0, s1 = sum g, s2 = sum g xhat (xhat = (y - mean) rstd), dy = rstd (g - s1/M - xhat s2/M),
    dbeta_out = dbeta_in + s1.  mean / rstd: the float32 values handed to the kernel, promoted.  mask: bool [M, C] or None."""
    da, y, mean, rstd = da.double(), y.double(), mean.double(), rstd.double()
    g = da if mask is None else torch.where(mask, da, torch.zeros((), dtype=torch.float64))
    xh = (y - mean) * rstd
    s1, s2 = g.sum(0), (g * xh).sum(0)
    dy = rstd * (g - s1 / M - xh * (s2 / M))
    return dy, torch.as_tensor(dbeta_in, dtype=torch.float64) + s1


def mask_from_activation(a):
    return a.double() > 0


def mask_from_y(y, mean, rstd, beta):
    return (y.double() - mean.double()) * rstd.double() + beta.double() > 0


def mask_from_threshold(y, thr):
    return y.double() > thr.double()


# ------------------------------------------------------------------------------------------------ shared case tables
# name, N, H, W, Cin, Cout, R, S, stride, (pt, pl, pb, pr): the GEOMS of tests/test_gpu_conv.py (same numbers) + the head
GEOMS = {
    "1x1_320_96": (2, 35, 35, 320, 96, 1, 1, 1, (0, 0, 0, 0)),
    "1x1_1088_320": (3, 17, 17, 1088, 320, 1, 1, 1, (0, 0, 0, 0)),
    "3x3_same_32_48": (2, 35, 35, 32, 48, 3, 3, 1, (1, 1, 1, 1)),
    "3x3_valid_s2_stem": (2, 31, 31, 8, 32, 3, 3, 2, (0, 0, 0, 0)),
    "3x3_valid_80_192": (1, 21, 21, 80, 192, 3, 3, 1, (0, 0, 0, 0)),
    "1x7_128_160": (2, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)),
    "7x1_160_192": (2, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)),
    "5x5_48_64": (1, 35, 35, 48, 64, 5, 5, 1, (2, 2, 2, 2)),
    "3x3_s2_same_asym": (4, 8, 8, 256, 256, 3, 3, 2, (0, 0, 1, 1)),
    "3x3_s2_valid_320_384": (2, 35, 35, 320, 384, 3, 3, 2, (0, 0, 0, 0)),
    "2x2_valid_128_96": (4, 4, 4, 128, 96, 2, 2, 1, (0, 0, 0, 0)),
    "1x3_192_224": (4, 8, 8, 192, 224, 1, 3, 1, (0, 1, 0, 1)),
    "head_25": (4, 6, 6, 96, 25, 1, 1, 1, (0, 0, 0, 0)),
}
SINGLE_WGRAD = ["3x3_same_32_48", "3x3_valid_s2_stem", "1x7_128_160", "5x5_48_64", "3x3_s2_same_asym", "2x2_valid_128_96",
                "1x1_320_96", "head_25"]
GROUP_PLAN_A = list(GEOMS)                                                   # the job list of the grouped-launch test
GROUP_PLAN_B = ["b35_3x3_alone"]
GEOMS_B = {"b35_3x3_alone": (8, 35, 35, 32, 32, 3, 3, 1, (1, 1, 1, 1))}
# (geometry, tile_config) of the statistics cases: a1 / a3 / a5 / a6 of test_conv_stats_atomic_rows + one resident-image case
STATS_CASES = {
    "igemm3": ((3, 35, 35, 64, 96, 3, 3, 1, (1, 1, 1, 1)), 0),
    "igemm5_128x128": ((3, 17, 17, 384, 320, 1, 1, 1, (0, 0, 0, 0)), 34),
    "direct3": ((2, 60, 60, 32, 32, 3, 3, 1, (0, 0, 0, 0)), 96),
    "split_k": ((8, 8, 8, 1536, 96, 3, 3, 1, (1, 1, 1, 1)), 128 + 6),
    "resident": ((3, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), 98),
}
BWD_STATS_GEOM = (3, 17, 17, 160, 96, 7, 1, 1, (3, 0, 3, 0))                 # test_conv_bn_bwd_stats_epilogue
FUSED_EXACT = ((64, 8, 8, 448, 2080, 1, 1, 1, (0, 0, 0, 0)), 33, 0, (192, 256))     # b8up of FUSED_BWD_CASES
BN_ROW_SHAPES = [(7, 8), (1001, 24), (2450, 96), (18496, 160)]               # the test_bn_backward_onepass shapes


def geom(name):
    return GEOMS[name] if name in GEOMS else GEOMS_B[name]


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """Integer inputs and exact references of one geometry: x, dy; w (forward, <= 5 taps per output channel) and y = conv(x, w);
    wd (data gradient, <= 8 taps per input channel) and dx; dw, db.  All int64 (the float64 references are integers)."""
    g = geom(name)
    N, H, W, Ci, Co, R, S, st, pads = g
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    x = int_tensor((N, H, W, Ci))
    dy = int_tensor((N, Ho, Wo, Co), coef=(2, 3, 11, 7), mod=5, off=2, salt=1)
    w = sparse_filter(Co, R, S, Ci)
    wd = sparse_filter_dgrad(Co, R, S, Ci)
    dw, db = conv_wgrad_ref(x, dy, R, S, st, pads)
    return dict(g=g, Ho=Ho, Wo=Wo, x=x, dy=dy, w=w, wd=wd, y=conv_forward_ref(x, w, st, pads).round().long(),
                dx=conv_dgrad_ref(wd, dy, (N, H, W, Ci), st, pads).round().long(), dw=dw.round().long(), db=db.round().long())


@functools.lru_cache(maxsize=None)
def forward_case(name, table):
    """x, w, y only (the statistics cases: no gradients needed)."""
    g = STATS_CASES[name][0] if table == "stats" else BWD_STATS_GEOM
    N, H, W, Ci, Co, R, S, st, pads = g
    x = int_tensor((N, H, W, Ci))
    w = sparse_filter(Co, R, S, Ci)
    return dict(g=g, x=x, w=w, y=conv_forward_ref(x, w, st, pads).round().long())


@functools.lru_cache(maxsize=None)
def bn_exact_case(M=256, Cc=64):
    """The exact tier: integer da / y, integer mean, rstd = 0.5, half-integer beta -- xhat, the sums and sums / M (M a power of
    two) are dyadic with few bits, so every float32 operation of every kernel form is exact."""
    y = int_tensor((M, Cc), mod=7, off=3)
    da = int_tensor((M, Cc), coef=(2, 3, 11, 7), mod=5, off=2, salt=2)
    c = torch.arange(Cc)
    mean = (c % 3 - 1).double()
    rstd = torch.full((Cc,), 0.5, dtype=torch.float64)
    beta = (c % 4 - 2).double() + 0.5
    return dict(y=y, da=da, mean=mean, rstd=rstd, beta=beta, thr=mean - beta / rstd)


@functools.lru_cache(maxsize=None)
def fused_exact_case():
    """The fused batch-norm tail on b8up: an integer upstream gradient through a sparse integer filter (<= 8 taps per input
    channel, |dyX| <= 2: |da| <= 16), rscale = 0."""
    g, cfg, cap, split = FUSED_EXACT
    N, H, W, Ci, Co, R, S, st, pads = g
    dyX = int_tensor((N, H, W, Co), coef=(2, 3, 11, 7), mod=5, off=2, salt=1)
    wd = sparse_filter_dgrad(Co, R, S, Ci)
    da = conv_dgrad_ref(wd, dyX, (N, H, W, Ci), st, pads).round().long()
    return dict(g=g, cfg=cfg, cap=cap, split=split, dyX=dyX, wd=wd, da=da)


def filter_coverage():
    """(label, k_coverage) of every filter the exact GPU tests use."""
    out = []
    for name in SINGLE_WGRAD:
        if name != "head_25":
            c = conv_case(name)
            out.append((name + " w", k_coverage(c["w"], min(8, c["w"][0].numel() // 4))))
            out.append((name + " wd", k_coverage(c["wd"], 8, transposed=True)))
    for name in STATS_CASES:
        out.append((name + " w", k_coverage(forward_case(name, "stats")["w"], 16)))
    out.append(("bn_bwd_stats w", k_coverage(forward_case("bw", "bwd_stats")["w"])))
    out.append(("fused wd", k_coverage(fused_exact_case()["wd"], 8, transposed=True)))
    return out


def exact_magnitudes():
    """(label, max |reference|, limit) for every reference the exact GPU tests compare with -- the same case tables."""
    out = []
    for name in sorted(set(SINGLE_WGRAD + GROUP_PLAN_A)) + GROUP_PLAN_B:
        c = conv_case(name)
        out.append((name + " dw x2", 2 * int(c["dw"].abs().max()), EXACT_LIMIT))        # (the second, accumulating launch)
        out.append((name + " db x2", 2 * int(c["db"].abs().max()), EXACT_LIMIT))
        if name in SINGLE_WGRAD and name != "head_25":
            out.append((name + " y", int(c["y"].abs().max()), BF16_INT_LIMIT))
            out.append((name + " dx", int(c["dx"].abs().max()), BF16_INT_LIMIT))
    for name in STATS_CASES:
        y = forward_case(name, "stats")["y"]
        out.append((name + " y", int(y.abs().max()), BF16_INT_LIMIT))
        out.append((name + " sum y^2", int((y * y).reshape(-1, y.shape[-1]).sum(0).max()), EXACT_LIMIT))
    y = forward_case("bw", "bwd_stats")["y"]
    out.append(("bn_bwd_stats 2 sum |g y|", 2 * 3 * int(y.abs().reshape(-1, y.shape[-1]).sum(0).max()), EXACT_LIMIT))
    e = bn_exact_case()
    out.append(("bn exact sum |da| |xhat| x2", 2 * int((e["da"].abs() * (e["y"].double() - e["mean"]).abs()).sum(0).max()), EXACT_LIMIT))
    f = fused_exact_case()
    out.append(("fused da", int(f["da"].abs().max()), 16))
    out.append(("fused sum |da| |xhat| x2", 8 * int(f["da"].abs().reshape(-1, f["da"].shape[-1]).sum(0).max()), EXACT_LIMIT))
    for M, Cc in BN_ROW_SHAPES:
        out.append(("rows M=%d" % M, M + 3, EXACT_LIMIT))
    return out
