"""GPU parity of the MFMA implicit-GEMM convolution kernels (forward, data gradient, weight
gradient) against a torch-CPU float32 convolution on the same bf16-rounded inputs.

Tolerance (bf16 in/out, fp32 accumulate): the kernel's result must be within ~1 bf16 ulp of
the float32 reference: |out - ref| <= 2^-7 |ref| + 2e-3 * max|ref|  (stated, used below);
float32 outputs (weight gradients, head outputs): rtol 2e-3 of max|ref|.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()
    return torch


def bf16_round(torch, t):
    return t.to(torch.bfloat16).to(torch.float32)


def ref_conv(torch, x, w, stride, pads):
    """x [N,H,W,C] f32, w [K,R,S,C] f32, pads (t,l,b,r) -> [N,Ho,Wo,K] f32 on CPU."""
    import torch.nn.functional as F
    xt = F.pad(x.permute(0, 3, 1, 2), (pads[1], pads[3], pads[0], pads[2]))
    return F.conv2d(xt, w.permute(0, 3, 1, 2), stride=stride).permute(0, 2, 3, 1).contiguous()


def close(torch, out, ref, f32=False):
    out, ref = out.float().cpu(), ref.float().cpu()
    mx = float(ref.abs().max()) + 1e-20
    if f32:
        err = float((out - ref).abs().max())
        return err <= 2e-3 * mx, "max err %.3g vs max|ref| %.3g" % (err, mx)
    bad = (out - ref).abs() > (2.0 ** -7) * ref.abs() + 2e-3 * mx
    return int(bad.sum()) == 0, "%d/%d out of tolerance, max err %.3g, max|ref| %.3g" % (
        int(bad.sum()), bad.numel(), float((out - ref).abs().max()), mx)


# name, N, H, W, Cin, Cout, R, S, stride, (pt, pl, pb, pr)
GEOMS = [
    ("1x1_320_96", 2, 35, 35, 320, 96, 1, 1, 1, (0, 0, 0, 0)),
    ("1x1_1088_320", 3, 17, 17, 1088, 320, 1, 1, 1, (0, 0, 0, 0)),
    ("3x3_same_32_48", 2, 35, 35, 32, 48, 3, 3, 1, (1, 1, 1, 1)),
    ("3x3_valid_s2_stem", 2, 31, 31, 8, 32, 3, 3, 2, (0, 0, 0, 0)),
    ("3x3_valid_80_192", 1, 21, 21, 80, 192, 3, 3, 1, (0, 0, 0, 0)),
    ("1x7_128_160", 2, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)),
    ("7x1_160_192", 2, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)),
    ("5x5_48_64", 1, 35, 35, 48, 64, 5, 5, 1, (2, 2, 2, 2)),
    ("3x3_s2_same_asym", 4, 8, 8, 256, 256, 3, 3, 2, (0, 0, 1, 1)),
    ("3x3_s2_valid_320_384", 2, 35, 35, 320, 384, 3, 3, 2, (0, 0, 0, 0)),
    ("2x2_valid_128_96", 4, 4, 4, 128, 96, 2, 2, 1, (0, 0, 0, 0)),
    ("1x3_192_224", 4, 8, 8, 192, 224, 1, 3, 1, (0, 1, 0, 1)),
    ("1x1_2080_1536_m4096", 64, 8, 8, 2080, 1536, 1, 1, 1, (0, 0, 0, 0)),
]


def out_hw(H, W, R, S, stride, pads):
    return (H + pads[0] + pads[2] - R) // stride + 1, (W + pads[1] + pads[3] - S) // stride + 1


def make_case(torch, g, seed=0):
    name, N, H, W, Ci, Co, R, S, st, pads = g
    gen = torch.Generator().manual_seed(seed)
    x = bf16_round(torch, torch.randn(N, H, W, Ci, generator=gen))
    w = bf16_round(torch, torch.randn(Co, R, S, Ci, generator=gen) / (R * S * Ci) ** 0.5)
    return x, w


@pytest.mark.parametrize("g", GEOMS, ids=[g[0] for g in GEOMS])
def test_conv_forward(T, g):
    torch = T
    from multibox_amd import ops
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    ref = ref_conv(torch, x, w, st, pads)
    # input lives in a channel slice of a wider buffer; output too
    xb = ops.View.alloc(N, H, W, Ci + 16, zero=True).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
    wd = w.to(torch.bfloat16).cuda().contiguous()
    d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb)
    rows = ops.conv_stats_rows(d)
    stats = torch.zeros((rows, Co, 2), dtype=torch.float32, device="cuda")
    d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=stats)
    ops.conv(d)
    torch.cuda.synchronize()
    out = yb.tensor()
    ok, msg = close(torch, out, ref)
    assert ok, msg
    # neighbours of the slice untouched
    full = yb.buf.reshape(N, Ho, Wo, Co + 24)
    assert float(full[..., :16].abs().max()) == 0 and float(full[..., 16 + Co:].abs().max()) == 0
    # batch-norm statistics partials: sums of the STORED (bf16) values
    st_sum = stats.sum(0).cpu()
    o32 = out.float().cpu().reshape(-1, Co)
    assert torch.allclose(st_sum[:, 0], o32.sum(0), rtol=1e-4, atol=1e-3 * float(o32.abs().sum(0).max()))
    assert torch.allclose(st_sum[:, 1], (o32 * o32).sum(0), rtol=1e-4)


def test_conv_epilogues(T):
    torch = T
    from multibox_amd import ops
    g = ("e", 2, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0))
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=3)
    gen = torch.Generator().manual_seed(4)
    scale = torch.rand(Co, generator=gen) + 0.5
    shift = torch.randn(Co, generator=gen)
    skip = bf16_round(torch, torch.randn(N, H, W, Co, generator=gen))
    ref = ref_conv(torch, x, w, st, pads)
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda()
    sc, sh = scale.cuda(), shift.cuda()
    # AFFINE + relu (frozen batch norm, detect.py:313-326)
    y = ops.View.alloc(N, H, W, Co)
    ops.conv(ops.make_desc(xb, wd, Co, R, S, st, 0, 0, y, epilogue=ops.EPI_AFFINE, relu=1, scale=sc, shift=sh))
    ok, msg = close(torch, y.tensor(), torch.relu(ref * scale + shift))
    assert ok, "affine: " + msg
    # RESIDUAL: relu(skip + 0.1*(acc + bias))  (model.py:39-43)
    sk = ops.View.alloc(N, H, W, Co + 8).slice(8, Co)
    sk.tensor().copy_(skip.to(torch.bfloat16))
    for relu in (1, 0):
        ops.conv(ops.make_desc(xb, wd, Co, R, S, st, 0, 0, y, epilogue=ops.EPI_RESIDUAL, relu=relu, shift=sh, skip=sk, rscale=0.1))
        r = skip + 0.1 * (ref + shift)
        ok, msg = close(torch, y.tensor(), torch.relu(r) if relu else r)
        assert ok, "residual relu=%d: %s" % (relu, msg)
    # accumulate (gradient summation into an existing bf16 buffer)
    y.tensor().copy_(skip.to(torch.bfloat16))
    ops.conv(ops.make_desc(xb, wd, Co, R, S, st, 0, 0, y, accumulate=1))
    ok, msg = close(torch, y.tensor(), skip + ref)
    assert ok, "accumulate: " + msg


def direct3_forward_with_stats(torch, g, before_launch=None):
    """Forward with statistics of descriptor g under tile_config 0 (implicit GEMM) and the direct 3x3 launch: outputs
    bit-identical, statistics = sums of the stored values, slices of wider buffers untouched outside, and within the file's
    tolerance of the float32 reference.  Returns what the callers go on with: x, w, the input view, the device filter, the
    last output view and the direct launch's statistics rows (= its grid).  before_launch(grid), if given, is called with
    that grid before anything is launched (a caller's reason to skip)."""
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=11)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    xb = ops.View.alloc(N, H, W, Ci + 16, zero=True).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    if before_launch is not None:
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], ops.View.alloc(N, Ho, Wo, Co))
        d.tile_config = ops.DIRECT3_TILE_CONFIG
        before_launch(ops.conv_stats_rows(d))
    outs = []
    for cfg in (0, ops.DIRECT3_TILE_CONFIG):
        yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb)
        d.tile_config = cfg
        rows = ops.conv_stats_rows(d)
        stats = torch.zeros((rows, Co, 2), dtype=torch.float32, device="cuda")
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=stats)
        d.tile_config = cfg
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        full = yb.buf.reshape(N, Ho, Wo, Co + 24)
        assert float(full[..., :16].abs().max()) == 0 and float(full[..., 16 + Co:].abs().max()) == 0
        outs.append((yb.tensor().clone(), stats.double().sum(0).cpu()))
    assert torch.equal(outs[0][0], outs[1][0]), float((outs[0][0].float() - outs[1][0].float()).abs().max())
    assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-3)
    ok, msg = close(torch, outs[1][0], ref_conv(torch, x, w, st, pads))
    assert ok, msg
    return x, w, xb, wd, yb, rows


@pytest.mark.parametrize("g", [("d1", 2, 37, 45, 32, 32, 3, 3, 1, (0, 0, 0, 0)), ("d2", 3, 41, 33, 32, 64, 3, 3, 1, (1, 1, 1, 1)),
                               ("d3", 2, 35, 35, 32, 48, 3, 3, 1, (1, 1, 1, 1)), ("d4", 2, 29, 50, 64, 32, 3, 3, 1, (1, 1, 1, 1)),
                               ("d5", 1, 20, 70, 64, 48, 3, 3, 1, (1, 1, 1, 1)), ("d6", 2, 24, 24, 32, 40, 3, 3, 1, (1, 1, 1, 1)),
                               ("d7", 4, 147, 147, 32, 64, 3, 3, 1, (1, 1, 1, 1)), ("d8", 3, 61, 75, 8, 32, 3, 3, 2, (0, 0, 0, 0)),
                               ("d9", 2, 40, 66, 8, 24, 3, 3, 2, (0, 0, 1, 1)), ("d10", 2, 299, 299, 8, 32, 3, 3, 2, (0, 0, 0, 0))],
                         ids=["valid_32_32", "same_32_64", "same_32_48", "same_64_32", "same_64_48", "cout_40", "stem_2b",
                              "first_layer_s2", "first_layer_s2_same_24", "stem_1a"])
def test_conv_direct3_bit_identical(T, g):
    """tile_config 96 (round 4, csrc/convd.hip; the last three cases: conv_stem_kernel, the stride-2 first layer on the packed
    RGB input): the direct 3x3 launch -- a persistent workgroup per CU stages each pixel
    patch with its halo once and multiplies the nine taps out of LDS -- against the implicit-GEMM launch of the same
    descriptor: forward with statistics and as a data gradient ("full" padding 2 for a VALID forward), ragged tile edges,
    more tiles than workgroups.  Same accumulation order: outputs bit-identical, statistics = sums of the stored values (one
    row per workgroup); slices of wider buffers untouched outside; what it does not cover is refused."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    stream = torch.cuda.current_stream().cuda_stream
    x, w, xb, wd, yb, _ = direct3_forward_with_stats(torch, g)
    # the affine (+ relu) epilogue of a folded batch norm (inference / --fine_tune forward): bit-identical to the implicit GEMM's
    gen = torch.Generator().manual_seed(7)
    scale, shift = (torch.rand(Co, generator=gen) + 0.5).cuda(), (torch.randn(Co, generator=gen) * 0.2).cuda()
    aff = []
    for cfg in (0, ops.DIRECT3_TILE_CONFIG):
        yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, epilogue=ops.EPI_AFFINE, relu=1, scale=scale, shift=shift)
        d.tile_config = cfg
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        aff.append(yb.tensor().clone())
    assert torch.equal(aff[0], aff[1]) and float(aff[1].float().min()) == 0.0 and float(aff[1].float().max()) > 0
    # data gradient of the same convolution: input = dy [N,Ho,Wo,Co], flipped / transposed filter, "full" padding R - 1 - pad
    gen = torch.Generator().manual_seed(5)
    if st == 1 and Co in (32, 64) and Ci <= 64 and not (Co == 64 and Ci > 48):
        dy = ops.View.alloc(N, Ho, Wo, Co)
        dy.tensor().copy_(torch.randn(N, Ho, Wo, Co, generator=gen).to(torch.bfloat16))
        wt = w.to(torch.bfloat16).flip(1, 2).permute(3, 1, 2, 0).contiguous().cuda()          # [Ci][R][S][Co]
        res = []
        for cfg in (0, ops.DIRECT3_TILE_CONFIG):
            gx = ops.View.alloc(N, H, W, Ci, zero=True)
            dd = ops.make_desc(dy, wt, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], gx, transposed=1)
            dd.tile_config = cfg
            assert l.mbx_conv(C.byref(dd), stream) == 0
            torch.cuda.synchronize()
            res.append(gx.tensor().clone())
        assert torch.equal(res[0], res[1]) and float(res[0].float().abs().max()) > 0
    # refused: a 1x1, a stride-2, an accumulate epilogue, 64 -> 64 channels
    bad = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, accumulate=1)
    bad.tile_config = ops.DIRECT3_TILE_CONFIG
    assert l.mbx_conv_supported(C.byref(bad)) == -2


@pytest.mark.parametrize("g", [("s1", 30, 50, 130, 32, 48, 3, 3, 1, (1, 1, 1, 1)), ("s2", 30, 50, 130, 64, 32, 3, 3, 1, (1, 1, 1, 1)),
                               ("s3", 30, 101, 261, 8, 32, 3, 3, 2, (0, 0, 0, 0))],
                         ids=["direct3_nbuf3", "direct3_nbuf2", "stem"])
def test_conv_direct_ring_steady_state(T, g):
    """The steady-state wait of the direct kernels' patch ring (a tile that is neither the workgroup's first nor in its tail) is
    taken only by a workgroup that walks at least four tiles at two tiles of look-ahead; the cases of
    test_conv_direct3_bit_identical reach two.  Here 7 x 5 x 30 = 1050 tiles of 8 x 32 (output 50 x 130: ragged right and
    bottom edges) on 256 workgroups: four and five tiles each.  Forward with statistics, bit-identical to the implicit GEMM.
    (On a quiet chip a wrong count need not show: test_deep_ring_bit_identical_under_memory_saturation is the proof under load.)"""
    torch = T
    name, N, H, W, Ci, Co, R, S, st, pads = g
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    ntiles = N * ((Ho + 7) // 8) * ((Wo + 31) // 32)      # the launch's 8 x 32 output tiles

    def walked(grid):                                     # (the library's grid, before anything is launched)
        ok = ntiles >= 4 * grid + 1 and ntiles % grid != 0
        if not ok and grid != 256:
            pytest.skip("%d tiles on %d workgroups: no workgroup with a first, a steady-state and a tail tile and an uneven "
                        "share (the cases are sized for 256 CUs)" % (ntiles, grid))
        assert ok, (ntiles, grid)

    direct3_forward_with_stats(torch, g, before_launch=walked)


@pytest.mark.parametrize("g,cfg", [(("a1", 3, 35, 35, 64, 96, 3, 3, 1, (1, 1, 1, 1)), 0), (("a2", 2, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), 10),
                                   (("a3", 3, 17, 17, 384, 320, 1, 1, 1, (0, 0, 0, 0)), 34), (("a4", 4, 35, 35, 320, 96, 1, 1, 1, (0, 0, 0, 0)), 35),
                                   (("a5", 2, 60, 60, 32, 32, 3, 3, 1, (0, 0, 0, 0)), 96), (("a6", 8, 8, 8, 1536, 96, 3, 3, 1, (1, 1, 1, 1)), 128 + 6)] +
                         [(("b%d" % c, 2, 8, 8, 96, 96, 3, 3, 1, (0, 0, 0, 0)), c) for c in list(range(1, 15)) + [33, 34, 35, 36, 37]] +
                         [(("c%d" % c, 5, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)), c) for c in list(range(1, 15)) + [33, 34, 35, 36, 37]],
                         ids=["igemm3", "igemm3_2deep", "igemm5_128x128", "igemm5_192x128", "direct3", "split_k"] +
                         ["small_cfg%d" % c for c in list(range(1, 15)) + [33, 34, 35, 36, 37]] +
                         ["mid_cfg%d" % c for c in list(range(1, 15)) + [33, 34, 35, 36, 37]])
def test_conv_stats_atomic_rows(T, g, cfg):
    """mbx_conv_desc.stats_rows_mod = 16 (round 4): the tiles ADD their statistics sums into 16 rows of a zeroed table
    (64-bit fixed-point integer atomics: order-independent) instead of writing a row each -- for every kernel family with a statistics epilogue.  Outputs
    bit-identical to the plain launch; the 16 rows sum to the plain rows' sums (float32 rounding of a different grouping:
    rtol 1e-5); with stats_ld the sums land in a channel slice of a wider table, the rest of which stays zero; and
    mbx_bn_apply_fused_mapped on the 16 rows gives mean / rstd / activation of finalize + apply on the plain rows."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=3)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    stream = torch.cuda.current_stream().cuda_stream
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    M = N * Ho * Wo
    ws = None

    def run(stats, mod, ld):
        nonlocal ws
        yb = ops.View.alloc(N, Ho, Wo, Co, zero=True)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=stats, stats_rows_mod=mod, stats_ld=ld)
        d.tile_config = cfg
        if cfg > 128:
            ws = torch.empty(int(l.mbx_conv_splitk_workspace_bytes(C.byref(d))) // 4, dtype=torch.float32, device="cuda")
            d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
        assert l.mbx_conv_supported(C.byref(d)) == 0
        assert mod == 0 or ops.conv_stats_rows(d) == mod
        ops.conv(d)
        torch.cuda.synchronize()
        return yb, d

    d0 = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], ops.View.alloc(N, Ho, Wo, Co))
    d0.tile_config = cfg
    rows = ops.conv_stats_rows(d0)
    plain = torch.zeros((rows, Co, 2), dtype=torch.float32, device="cuda")
    y0, _ = run(plain, 0, 0)
    ld = Co + 24
    table = torch.zeros((16, ld, 2), dtype=torch.int64, device="cuda")      # fixed point, units of 2^-20 (integer atomics)
    y1, _ = run(table[:, 8:], 16, ld)                 # the member's first channel = channel 8 of the table
    assert torch.equal(y0.tensor(), y1.tensor())
    assert int(table[:, :8].abs().max()) == 0 and int(table[:, 8 + Co:].abs().max()) == 0
    want, got = plain.double().sum(0).cpu(), table[:, 8:8 + Co].sum(0).double().cpu() / 2.0 ** 20
    assert torch.allclose(want, got, rtol=1e-5, atol=1e-3), float((want - got).abs().max())
    assert int((table[:, 8:8 + Co, 1].abs().sum(1) > 0).sum()) == min(16, rows)       # spread over the rows, not piled on one
    # integer adds are associative: a second launch into a cleared table leaves the same bits whatever order the tiles arrive in
    first = table.clone()
    table.zero_()
    run(table[:, 8:], 16, ld)
    assert torch.equal(first, table)
    # the consumer: finalize + apply on the plain rows against the one-launch form on the 16 rows
    dense = table[:, 8:8 + Co].contiguous()
    beta = (torch.randn(Co, generator=torch.Generator().manual_seed(1)) * 0.3).cuda()
    outs = []
    for fused in (False, True):
        mean, rstd = torch.zeros(Co, device="cuda"), torch.zeros(Co, device="cuda")
        mm, mv = torch.zeros(Co, device="cuda"), torch.ones(Co, device="cuda")
        a = ops.View.alloc(N, Ho, Wo, Co + 16, zero=True)
        thr = torch.zeros(Co, device="cuda")
        if fused:
            cm = _lib.ChanMap()
            cm.n, cm.c_begin[0], cm.offset[0], cm.c_begin[1], cm.offset[1] = 2, 0, 0, 8, 16      # channels >= 8 shifted by 16
            assert l.mbx_bn_apply_fused_mapped(dense.data_ptr(), 16, M, 0.001, -1.0, y1.ptr, M, Co, beta.data_ptr(), 1, a.ptr, a.ld,
                                               C.byref(cm), mean.data_ptr(), rstd.data_ptr(), mm.data_ptr(), mv.data_ptr(),
                                               thr.data_ptr(), stream) == 0
        else:
            assert l.mbx_bn_finalize(plain.data_ptr(), rows, Co, M, 0.001, -1.0, mean.data_ptr(), rstd.data_ptr(), mm.data_ptr(),
                                     mv.data_ptr(), stream) == 0
            cm = _lib.ChanMap()
            cm.n, cm.c_begin[0], cm.offset[0], cm.c_begin[1], cm.offset[1] = 2, 0, 0, 8, 16
            assert l.mbx_bn_apply_mapped(y0.ptr, M, Co, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr(), 1, a.ptr, a.ld,
                                         C.byref(cm), stream) == 0
        torch.cuda.synchronize()
        outs.append((mean.cpu(), rstd.cpu(), mm.cpu(), mv.cpu(), a.buf.float().cpu().reshape(-1, Co + 16), thr.cpu()))
    for i in range(4):
        assert torch.allclose(outs[0][i], outs[1][i], rtol=2e-5, atol=1e-6), i
    ok, msg = close(torch, outs[1][4], outs[0][4])
    assert ok, msg
    assert float(outs[1][4][:, 8:24].abs().max()) == 0                                  # the hole the map leaves
    thr_ref = outs[1][0] - beta.cpu() / outs[1][1]
    assert torch.allclose(outs[1][5], thr_ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("cfg", [0, 33, 96, 98])
def test_conv_stats_fixed_point_out_of_range_poisons(T, cfg):
    """the 64-bit fixed-point statistics rows (stats_rows_mod > 0) are exact while a tile sum stays
    below 2^41; beyond that -- activations of ~1e8 and ~1e16, as `--fine_tune` straight after a fresh start produces them, or
    a NaN -- the conversion used to wrap into FINITE garbage.  Now: in range (inputs ~1e3) the one-launch consumer agrees with
    finalize on the float32 rows; out of range the channel is POISONED (negative sum-of-squares word) and
    mbx_bn_apply_fused_mapped returns NaN mean / rstd / activations for it -- never finite values that are wrong -- whatever
    kernel family wrote the rows (implicit GEMM, persistent, direct, resident image); the other channels stay exact."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    g = {0: ("s", 3, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), 33: ("s", 3, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)),
         96: ("s", 2, 150, 150, 32, 32, 3, 3, 1, (1, 1, 1, 1)), 98: ("s", 40, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3))}[cfg]
    name, N, H, W, Ci, Co, R, S, st, pads = g
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    M = N * Ho * Wo
    stream = torch.cuda.current_stream().cuda_stream
    x, w = make_case(torch, g, seed=5)
    wd = w.to(torch.bfloat16).cuda().contiguous()
    beta = torch.zeros(Co, device="cuda")
    # (1e4 .. 1e6: ADVICE round 5 -- the window in which single tile sums are in range but the TOTAL of a row's adders, or the
    # consumer's sum over the rows, used to wrap: every adder is now held to its share of the total range, include/mbx.h)
    for scale, hot in ((1e3, None), (1e3, 5), (1e4, 5), (1e5, 5), (1e6, 5), (1e8, 5), (1e16, 5), (float("nan"), 5)):
        xs = x.clone()
        if hot is None:
            xs *= scale
        else:
            # only the weights of output channel `hot` see the huge / NaN values: input channel 0 is large, its weight non-zero there
            xs[..., 0] = scale if scale == scale else float("nan")
            wz = w.clone(); wz[:, :, :, 0] = 0.0; wz[hot, :, :, 0] = 1.0
            wd = wz.to(torch.bfloat16).cuda().contiguous()
        xb = ops.View.alloc(N, H, W, Ci)
        xb.tensor().copy_(xs.to(torch.bfloat16))
        yb = ops.View.alloc(N, Ho, Wo, Co, zero=True)
        table = torch.zeros((8, Co, 2), dtype=torch.int64, device="cuda")
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=table, stats_rows_mod=8, stats_ld=Co)
        d.tile_config = cfg
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        mean, rstd = torch.zeros(Co, device="cuda"), torch.zeros(Co, device="cuda")
        a = ops.View.alloc(N, Ho, Wo, Co, zero=True)
        assert l.mbx_bn_apply_fused_mapped(table.data_ptr(), 8, M, 0.001, -1.0, yb.ptr, M, Co, beta.data_ptr(), 0, a.ptr, a.ld,
                                           None, mean.data_ptr(), rstd.data_ptr(), None, None, None, stream) == 0
        torch.cuda.synchronize()
        y64 = yb.tensor().double().reshape(M, Co)
        want_mean = y64.mean(0)
        want_rstd = 1.0 / torch.sqrt(y64.var(0, unbiased=False) + 0.001)
        ok = torch.ones(Co, dtype=torch.bool, device="cuda")
        if scale != scale:
            # a NaN input reaches EVERY output channel (0 x NaN = NaN): all of them are poisoned, none reports a finite statistic
            assert bool(torch.isnan(mean).all()) and bool(torch.isnan(rstd).all()) and int(table[:, :, 1].min(0).values.max()) < 0
            continue
        if hot is not None:
            ok[hot] = False
            # the hot channel is EITHER exact (its total sum of squares below 2^42) OR poisoned -- never finite and wrong
            in_range = float((y64[:, hot] ** 2).sum()) < 2.0 ** 42 and float(y64[:, hot].abs().sum()) < 2.0 ** 42
            if bool(torch.isnan(mean[hot])):
                assert bool(torch.isnan(rstd[hot])) and bool(torch.isnan(a.tensor().float()[..., hot]).all())
                assert int(table[:, hot, 1].min()) < 0
                # (an adder is held to its SHARE of the range, so the poison may come early by up to the adder count -- never late)
                tot = max(float((y64[:, hot] ** 2).sum()), float(y64[:, hot].abs().sum()))
                assert tot >= 2.0 ** 42 / 64, (scale, tot, "poisoned although far inside the documented range")
            else:
                assert in_range, (scale, float(mean[hot]), "finite statistics for a channel whose total is out of range")
                assert abs(float(mean[hot]) - float(want_mean[hot])) <= 1e-4 * abs(float(want_mean[hot])) + 1e-3
                assert abs(float(rstd[hot]) - float(want_rstd[hot])) <= 1e-4 * float(want_rstd[hot])
            if scale >= 1e8:
                assert bool(torch.isnan(mean[hot]))
        assert torch.allclose(mean[ok].double(), want_mean[ok], rtol=1e-4, atol=1e-4 * float(want_mean[ok].abs().max()))
        assert torch.allclose(rstd[ok].double(), want_rstd[ok], rtol=1e-4)
        assert bool(torch.isfinite(a.tensor().float()[..., ok]).all())


@pytest.mark.parametrize("g", [("w1", 3, 35, 35, 32, 32, 3, 3, 1, (1, 1, 1, 1)), ("w2", 2, 35, 35, 32, 48, 3, 3, 1, (1, 1, 1, 1)),
                               ("w3", 2, 35, 35, 48, 64, 3, 3, 1, (1, 1, 1, 1)), ("w4", 2, 35, 35, 64, 48, 3, 3, 1, (1, 1, 1, 1)),
                               ("w5", 3, 35, 35, 48, 32, 3, 3, 1, (1, 1, 1, 1)), ("w6", 2, 19, 17, 32, 40, 3, 3, 1, (0, 0, 0, 0)),
                               ("w7", 5, 33, 60, 64, 32, 3, 3, 1, (1, 1, 1, 1)), ("w8", 64, 35, 35, 48, 64, 3, 3, 1, (1, 1, 1, 1))],
                         ids=["32_32", "32_48", "48_64", "64_48", "48_32", "valid_17wide_cout40", "60wide_64_32", "block35_0c_b64"])
def test_conv_directw_bit_identical(T, g):
    """tile_config 97 (round 4, csrc/convd.hip conv_directw_kernel): the direct 3x3 launch with WHOLE-WIDTH tiles for narrow maps
    (block35's 35 x 35 layers) -- TH rows of the map per tile, the K range walked linearly in the implicit GEMM's 32-element
    groups (C_in 48: a group straddles two taps) -- against the implicit-GEMM launch of the same descriptor: forward with
    statistics, affine + relu, and as a data gradient; ragged last tile, more tiles than workgroups (BATCH_SIZE 64).
    Outputs bit-identical; statistics = sums of the stored values; slices of wider buffers untouched outside."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=13)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    stream = torch.cuda.current_stream().cuda_stream
    xb = ops.View.alloc(N, H, W, Ci + 16, zero=True).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    outs = []
    for cfg in (0, ops.DIRECTW_TILE_CONFIG):
        yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb)
        d.tile_config = cfg
        rows = ops.conv_stats_rows(d)
        stats = torch.zeros((rows, Co, 2), dtype=torch.float32, device="cuda")
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=stats)
        d.tile_config = cfg
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        full = yb.buf.reshape(N, Ho, Wo, Co + 24)
        assert float(full[..., :16].abs().max()) == 0 and float(full[..., 16 + Co:].abs().max()) == 0
        outs.append((yb.tensor().clone(), stats.double().sum(0).cpu()))
    assert torch.equal(outs[0][0], outs[1][0]), float((outs[0][0].float() - outs[1][0].float()).abs().max())
    assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-3)
    if N <= 8:
        ok, msg = close(torch, outs[1][0], ref_conv(torch, x, w, st, pads))
        assert ok, msg
    gen = torch.Generator().manual_seed(7)
    scale, shift = (torch.rand(Co, generator=gen) + 0.5).cuda(), (torch.randn(Co, generator=gen) * 0.2).cuda()
    aff = []
    for cfg in (0, ops.DIRECTW_TILE_CONFIG):
        yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, epilogue=ops.EPI_AFFINE, relu=1, scale=scale, shift=shift)
        d.tile_config = cfg
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        aff.append(yb.tensor().clone())
    assert torch.equal(aff[0], aff[1]) and float(aff[1].float().max()) > 0
    # data gradient: input = dy [N,Ho,Wo,Co], flipped / transposed filter, "full" padding R - 1 - pad
    if Co in (32, 48, 64) and not (Co == 64 and Ci > 48):
        dy = ops.View.alloc(N, Ho, Wo, Co)
        dy.tensor().copy_(torch.randn(N, Ho, Wo, Co, generator=gen).to(torch.bfloat16))
        wt = w.to(torch.bfloat16).flip(1, 2).permute(3, 1, 2, 0).contiguous().cuda()          # [Ci][R][S][Co]
        res = []
        for cfg in (0, ops.DIRECTW_TILE_CONFIG):
            gx = ops.View.alloc(N, H, W, Ci, zero=True)
            dd = ops.make_desc(dy, wt, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], gx, transposed=1)
            dd.tile_config = cfg
            assert l.mbx_conv(C.byref(dd), stream) == 0
            torch.cuda.synchronize()
            res.append(gx.tensor().clone())
        assert torch.equal(res[0], res[1]) and float(res[0].float().abs().max()) > 0
    bad = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, accumulate=1)
    bad.tile_config = ops.DIRECTW_TILE_CONFIG
    assert l.mbx_conv_supported(C.byref(bad)) == -2


@pytest.mark.parametrize("g", [("r1", 3, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), ("r2", 3, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)),
                               ("r3", 5, 12, 15, 128, 160, 1, 7, 1, (0, 3, 0, 3)), ("r4", 2, 9, 11, 160, 192, 7, 1, 1, (3, 0, 3, 0)),
                               ("r5", 64, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), ("r6", 64, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)),
                               ("r7", 70, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)), ("r8", 5, 8, 8, 192, 224, 1, 3, 1, (0, 1, 0, 1)),
                               ("r9", 64, 8, 8, 224, 256, 3, 1, 1, (1, 0, 1, 0)), ("r10", 70, 8, 8, 192, 224, 1, 3, 1, (0, 1, 0, 1)),
                               ("r11", 150, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), ("r12", 256, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)),
                               ("r13", 256, 8, 8, 224, 256, 3, 1, 1, (1, 0, 1, 0)), ("r14", 256, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)),
                               ("r15", 300, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3))],
                         ids=["1x7_128_160", "7x1_160_192", "1x7_12x15", "7x1_9x11", "1x7_b64", "7x1_b64", "7x1_b70_two_tiles_per_wg",
                              "block8_1x3_192_224", "block8_3x1_224_256_b64", "block8_1x3_b70_two_tiles_per_wg",
                              "1x7_b150_three_tiles_across_images", "7x1_b256_image_per_wg", "block8_3x1_b256_image_per_wg",
                              "1x7_b256_image_per_wg", "1x7_b300_ragged_tiles_per_wg"])
def test_conv_resident_bit_identical(T, g):
    """tile_config 98 (round 5, csrc/convr.hip conv_resident_kernel): block17's 1x7 / 7x1 layers (model.py:33-37) with the whole
    input image of a tile resident in LDS and the filter streamed per tap -- against the implicit-GEMM launch of the same
    descriptor: forward with statistics (plain rows and the 8 integer-atomic rows), affine + relu, and as a data gradient
    (160 -> 128 and 192 -> 160 channels); smaller maps, more tiles than workgroups.  Outputs bit-identical; statistics =
    sums of the stored values; slices of wider buffers untouched outside."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=17)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    stream = torch.cuda.current_stream().cuda_stream
    xb = ops.View.alloc(N, H, W, Ci + 16, zero=True).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    outs = []
    for cfg in (0, ops.RESIDENT_TILE_CONFIG):
        yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb)
        d.tile_config = cfg
        rows = ops.conv_stats_rows(d)
        assert cfg == 0 or rows == N
        stats = torch.zeros((rows, Co, 2), dtype=torch.float32, device="cuda")
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=stats)
        d.tile_config = cfg
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        full = yb.buf.reshape(N, Ho, Wo, Co + 24)
        assert float(full[..., :16].abs().max()) == 0 and float(full[..., 16 + Co:].abs().max()) == 0
        # the 8 integer-atomic rows (the training default): order-independent, so the two launches agree to the last bit
        st8 = torch.zeros((8, Co, 2), dtype=torch.int64, device="cuda")
        d8 = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=st8, stats_rows_mod=8, stats_ld=Co)
        d8.tile_config = cfg
        ops.conv(d8)
        torch.cuda.synchronize()
        outs.append((yb.tensor().clone(), stats.double().sum(0).cpu(), st8.sum(0).cpu()))
    assert torch.equal(outs[0][0], outs[1][0]), float((outs[0][0].float() - outs[1][0].float()).abs().max())
    assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-3)
    o64 = outs[1][0].double().cpu().reshape(-1, Co)
    assert torch.allclose(outs[1][1][:, 0], o64.sum(0), rtol=1e-5, atol=1e-3) and torch.allclose(outs[1][1][:, 1], (o64 * o64).sum(0), rtol=1e-5)
    assert torch.allclose(outs[0][2].double(), outs[1][2].double(), rtol=1e-6, atol=64.0)      # fixed point, 2^-20 units: per-tile roundings differ
    if N <= 8:
        ok, msg = close(torch, outs[1][0], ref_conv(torch, x, w, st, pads))
        assert ok, msg
    gen = torch.Generator().manual_seed(7)
    scale, shift = (torch.rand(Co, generator=gen) + 0.5).cuda(), (torch.randn(Co, generator=gen) * 0.2).cuda()
    aff = []
    for cfg in (0, ops.RESIDENT_TILE_CONFIG):
        yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, epilogue=ops.EPI_AFFINE, relu=1, scale=scale, shift=shift)
        d.tile_config = cfg
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        aff.append(yb.tensor().clone())
    assert torch.equal(aff[0], aff[1]) and float(aff[1].float().max()) > 0
    # data gradient: input = dy [N,Ho,Wo,Co], flipped / transposed filter, "full" padding R - 1 - pad
    dy = ops.View.alloc(N, Ho, Wo, Co + 32).slice(32, Co)
    dy.tensor().copy_(torch.randn(N, Ho, Wo, Co, generator=gen).to(torch.bfloat16))
    wt = w.to(torch.bfloat16).flip(1, 2).permute(3, 1, 2, 0).contiguous().cuda()          # [Ci][R][S][Co]
    res = []
    for cfg in (0, ops.RESIDENT_TILE_CONFIG):
        gx = ops.View.alloc(N, H, W, Ci + 8, zero=True).slice(8, Ci)
        dd = ops.make_desc(dy, wt, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], gx, transposed=1)
        dd.tile_config = cfg
        assert l.mbx_conv(C.byref(dd), stream) == 0
        torch.cuda.synchronize()
        assert float(gx.buf.reshape(N, H, W, Ci + 8)[..., :8].abs().max()) == 0
        res.append(gx.tensor().clone())
    assert torch.equal(res[0], res[1]) and float(res[0].float().abs().max()) > 0
    bad = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, accumulate=1)
    bad.tile_config = ops.RESIDENT_TILE_CONFIG
    assert l.mbx_conv_supported(C.byref(bad)) == -2


@pytest.mark.parametrize("cfg", [0, 2, 5, 6, 10, 12, 14, 33, 34, 35, 37, "pair"])
def test_conv_bn_bwd_stats_epilogue(T, cfg):
    """mbx_conv_desc.bn_bwd_stats (round 4): the data gradient that writes an activation gradient also adds the batch-norm
    backward sums {sum g, sum g y}, g = (y > thr) ? stored gradient : 0, of the layers that own its output channels -- two
    table entries here (channels [0, 64) -> columns 16.. of a 96-wide y, [64, 96) -> a 32-wide y), 8 rows.  Outputs
    bit-identical to the plain launch; sums = float64 sums of the same expression (rtol 1e-4); the rest of the tables
    untouched; mbx_bn_bwd_apply_rows on them = the three-launch backward (reduce / finalize / apply) on the same tensors to
    1 bf16 ulp, dbeta to 1e-4.  The 256 x 128 persistent tile refuses the table (no such instantiation: registers)."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    g = ("bw", 3, 17, 17, 160, 96, 7, 1, 1, (3, 0, 3, 0))
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=9)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    M = N * Ho * Wo
    stream = torch.cuda.current_stream().cuda_stream
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    gen = torch.Generator().manual_seed(4)
    Y0 = (torch.randn(M, 96, generator=gen) * 1.5 + 0.3).to(torch.bfloat16).cuda()
    Y1 = (torch.randn(M, 32, generator=gen) * 0.7 - 0.2).to(torch.bfloat16).cuda()
    thr0 = (torch.randn(96, generator=gen) * 0.5).cuda()
    thr1 = (torch.randn(32, generator=gen) * 0.5).cuda()
    thr1[:8] = float("-inf")                                           # (a layer without relu: everything passes)
    st0 = torch.zeros((8, 96, 2), dtype=torch.float32, device="cuda")
    st1 = torch.zeros((8, 48, 2), dtype=torch.float32, device="cuda")
    tab = _lib.BnBwdStats()
    tab.n, tab.rows_mod = 2, 8
    tab.c_begin[0], tab.c_begin[1] = 0, 64
    tab.y[0], tab.ld_y[0], tab.relu_thr[0], tab.stats[0], tab.stats_ld[0] = Y0.data_ptr() + 2 * 16, 96, thr0.data_ptr() + 4 * 16, st0.data_ptr() + 8 * 16, 96
    tab.y[1], tab.ld_y[1], tab.relu_thr[1], tab.stats[1], tab.stats_ld[1] = Y1.data_ptr(), 32, thr1.data_ptr(), st1.data_ptr() + 8 * 8, 48

    def desc(yb, table):
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, rscale=0.17)
        d.tile_config = 0 if cfg == "pair" else cfg
        if table:
            d.bn_bwd_stats = C.addressof(tab)
        return d

    ya, yb_ = ops.View.alloc(N, Ho, Wo, Co, zero=True), ops.View.alloc(N, Ho, Wo, Co, zero=True)
    ops.conv(desc(ya, False))
    if cfg == "pair":
        # two problems in one grid: the second one a plain copy of the first into another buffer (its own table: rows of st0 / st1 too)
        yc = ops.View.alloc(N, Ho, Wo, Co, zero=True)
        d1, d2 = desc(yb_, True), desc(yc, True)
        d1.tile_config = d2.tile_config = 10
        assert l.mbx_conv_pair(C.byref(d1), C.byref(d2), stream) == 0
        scale = 2.0
    else:
        assert l.mbx_conv_supported(C.byref(desc(yb_, True))) == 0
        ops.conv(desc(yb_, True))
        scale = 1.0
    torch.cuda.synchronize()
    assert torch.equal(ya.tensor(), yb_.tensor())
    da = yb_.tensor().reshape(M, Co).float().cpu().double()
    for (Y, thr, tb, c_lo, c_n, y_lo, s_lo) in ((Y0, thr0, st0, 0, 64, 16, 16), (Y1, thr1, st1, 64, 32, 0, 8)):
        yy = Y[:, y_lo:y_lo + c_n].float().cpu().double()
        gg = torch.where(yy > thr[y_lo:y_lo + c_n].cpu().double(), da[:, c_lo:c_lo + c_n], torch.zeros(()).double())
        want = torch.stack([gg.sum(0), (gg * yy).sum(0)], 1) * scale
        got = tb[:, s_lo:s_lo + c_n].double().sum(0).cpu()
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-3 * float(want.abs().max())), (c_lo, float((got - want).abs().max()))
        assert float(tb[:, :s_lo].abs().max()) == 0 and float(tb[:, s_lo + c_n:].abs().max()) == 0
    # unsupported: the 256 x 128 persistent tile; an accumulate epilogue with the table is an argument error
    bad = desc(yb_, True)
    bad.tile_config = 36
    assert l.mbx_conv_supported(C.byref(bad)) == -2
    bad = desc(yb_, True)
    bad.accumulate = 1
    assert l.mbx_conv_supported(C.byref(bad)) == -1
    if cfg != 0:
        return
    # ---- the consumer: one streaming launch against the three-launch form, layer 0's 64 channels (y columns 16..80)
    Kc = 64
    yv = Y0[:, 16:16 + Kc].contiguous()
    yf = yv.float()
    mean = yf.mean(0).contiguous()
    rstd = torch.rsqrt(yf.var(0, unbiased=False) + 0.001).contiguous()
    beta = (torch.randn(Kc, generator=gen) * 0.3).cuda()
    thr = (mean - beta / rstd).contiguous()
    table = torch.zeros((8, Kc, 2), dtype=torch.float32, device="cuda")
    tab1 = _lib.BnBwdStats()
    tab1.n, tab1.rows_mod = 2, 8
    tab1.c_begin[0], tab1.c_begin[1] = 0, 64
    tab1.y[0], tab1.ld_y[0], tab1.relu_thr[0], tab1.stats[0], tab1.stats_ld[0] = yv.data_ptr(), Kc, thr.data_ptr(), table.data_ptr(), Kc
    tab1.y[1], tab1.ld_y[1], tab1.relu_thr[1], tab1.stats[1], tab1.stats_ld[1] = Y1.data_ptr(), 32, thr1.data_ptr(), st1.data_ptr() + 8 * 8, 48
    d = desc(yb_, False)
    d.bn_bwd_stats = C.addressof(tab1)
    ops.conv(d)
    dav = yb_.slice(0, Kc)                                             # the gradient view: channels [0, 64) of the 96-wide output
    outs = []
    for rows_form in (False, True):
        dbeta = torch.full((Kc,), 0.5, dtype=torch.float32, device="cuda")
        dy = torch.zeros((M, Kc), dtype=torch.bfloat16, device="cuda")
        if rows_form:
            assert l.mbx_bn_bwd_apply_rows(table.data_ptr(), 8, dav.ptr, dav.ld, yv.data_ptr(), M, Kc, mean.data_ptr(), rstd.data_ptr(),
                                           thr.data_ptr(), dbeta.data_ptr(), dy.data_ptr(), None, stream) == 0
        else:
            rows = l.mbx_bn_bwd_rows(M, Kc)
            part = torch.zeros((rows, Kc, 2), dtype=torch.float32, device="cuda")
            m12 = torch.zeros(2 * Kc, dtype=torch.float32, device="cuda")
            a = (dav.ptr, dav.ld, None, 0, 1, yv.data_ptr(), M, Kc, mean.data_ptr(), rstd.data_ptr(), beta.data_ptr())
            assert l.mbx_bn_bwd_reduce(*a, part.data_ptr(), stream) == 0
            assert l.mbx_bn_bwd_finalize(part.data_ptr(), rows, Kc, M, dbeta.data_ptr(), m12.data_ptr(), stream) == 0
            assert l.mbx_bn_bwd_apply(*a, m12.data_ptr(), dy.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        outs.append((dy.float().cpu(), dbeta.cpu()))
    ok, msg = close(torch, outs[1][0], outs[0][0])
    assert ok, msg
    assert torch.allclose(outs[1][1], outs[0][1], rtol=1e-4, atol=1e-4 * float(outs[0][1].abs().max()))


@pytest.mark.parametrize("cfg", [0, 10, 11, 5, 6])
def test_conv_pair_bit_identical(T, cfg):
    """mbx_conv_pair (round 4): two independent convolutions of different shape (block35's sibling 3x3 branches: 32 -> 32 and
    32 -> 48 channels on slices of one buffer; a 5x5 beside a 3x3) in ONE grid == two mbx_conv launches, bit for bit, forward
    with statistics and as data gradients; a configuration the pair kernels do not cover is refused (-2), nothing written."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    gen = torch.Generator().manual_seed(cfg + 3)
    N, H, W = 4, 35, 35
    zb = ops.View.alloc(N, H, W, 240, zero=True)
    zb.tensor().copy_(torch.randn(N, H, W, 240, generator=gen).to(torch.bfloat16))
    stream = torch.cuda.current_stream().cuda_stream
    shapes = [((0, 32), 32, 3, 3, 1), ((32, 32), 48, 5, 5, 2)]           # (input slice, C_out, R, S, pad)

    def descs(transposed):
        out = []
        for (c0, ci), co, R, S_, pad in shapes:
            if transposed:
                cin, cout = co, ci
                x = ops.View.alloc(N, H, W, cin, zero=True)
                x.tensor().copy_(torch.randn(N, H, W, cin, generator=torch.Generator().manual_seed(co)).to(torch.bfloat16))
            else:
                cin, cout, x = ci, co, zb.slice(c0, ci)
            w = (torch.randn(cout, R, S_, cin, generator=torch.Generator().manual_seed(co + R)) / (R * S_ * cin) ** 0.5).to(torch.bfloat16).cuda()
            ys = [ops.View.alloc(N, H, W, cout + 8, zero=True).slice(8, cout) for _ in range(2)]
            ds = []
            for y in ys:
                d = ops.make_desc(x, w, cout, R, S_, 1, pad, pad, y, transposed=transposed)
                d.tile_config = cfg
                stt = None
                if not transposed:
                    stt = torch.zeros((ops.conv_stats_rows(d) + 2, cout, 2), device="cuda")
                    d = ops.make_desc(x, w, cout, R, S_, 1, pad, pad, y, stats=stt)
                    d.tile_config = cfg
                ds.append((d, y, stt, x, w))
            out.append(ds)
        return out
    for transposed in (0, 1):
        (a0, a1), (b0, b1) = descs(transposed)
        rc = l.mbx_conv_pair(C.byref(a1[0]), C.byref(b1[0]), stream)
        torch.cuda.synchronize()
        if cfg == 6:                                                      # tile_config 6 = the eight-wave 256x128 tile: not a pair kernel
            assert rc == -2 and float(a1[1].tensor().float().abs().max()) == 0
            continue
        assert rc == 0
        assert l.mbx_conv(C.byref(a0[0]), stream) == 0 and l.mbx_conv(C.byref(b0[0]), stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(a0[1].tensor(), a1[1].tensor()) and torch.equal(b0[1].tensor(), b1[1].tensor())
        assert float(a0[1].tensor().float().abs().max()) > 0 and float(b0[1].tensor().float().abs().max()) > 0
        if not transposed:
            assert torch.equal(a0[2], a1[2]) and torch.equal(b0[2], b1[2])


@pytest.mark.parametrize("g", [("sk1", 16, 8, 8, 1536, 96, 3, 3, 1, (1, 1, 1, 1)), ("sk2", 16, 8, 8, 1536, 256, 3, 3, 2, (0, 0, 1, 1)),
                               ("sk3", 3, 9, 9, 200, 40, 3, 3, 1, (1, 1, 1, 1)), ("sk4", 2, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3))],
                         ids=["head_6x6", "head_s2", "ragged", "1x7"])
@pytest.mark.parametrize("S", [2, 5, 16])
def test_conv_split_k(T, g, S):
    """tile_config 128 + S (round 4): K slices as float32 partial tiles + one reduce launch that rounds, stores and writes the
    batch-norm statistics partials.  Against the float32 reference at the stated 1-bf16-ulp tolerance (the float32 sum is
    grouped differently from the one-pass kernels: NOT bit-identical to them, by design), statistics = sums of the STORED
    values, neighbours of the output slice untouched, a second launch bit-identical (fixed slice order: deterministic)."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S_, st, pads = g
    x, w = make_case(torch, g, seed=7)
    Ho, Wo = out_hw(H, W, R, S_, st, pads)
    ref = ref_conv(torch, x, w, st, pads)
    xb = ops.View.alloc(N, H, W, Ci + 16, zero=True).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    outs = []
    for rep in range(2):
        yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
        d = ops.make_desc(xb, wd, Co, R, S_, st, pads[0], pads[1], yb)
        d.tile_config = ops.SPLITK_FLAG + S
        rows = ops.conv_stats_rows(d)
        assert rows == (N * Ho * Wo + 15) // 16
        stats = torch.full((rows, Co, 2), float("nan"), dtype=torch.float32, device="cuda")
        d = ops.make_desc(xb, wd, Co, R, S_, st, pads[0], pads[1], yb, stats=stats)
        d.tile_config = ops.SPLITK_FLAG + S
        assert l.mbx_conv(C.byref(d), torch.cuda.current_stream().cuda_stream) == -4          # no workspace: MBX_ERR_WORKSPACE
        need = int(l.mbx_conv_splitk_workspace_bytes(C.byref(d)))
        assert need > 0
        ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device="cuda")
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), need
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        out = yb.tensor()
        ok, msg = close(torch, out, ref)
        assert ok, msg
        full = yb.buf.reshape(N, Ho, Wo, Co + 24)
        assert float(full[..., :16].abs().max()) == 0 and float(full[..., 16 + Co:].abs().max()) == 0
        st_sum = stats.sum(0).cpu()
        o32 = out.float().cpu().reshape(-1, Co)
        assert torch.allclose(st_sum[:, 0], o32.sum(0), rtol=1e-4, atol=1e-3 * float(o32.abs().sum(0).max()))
        assert torch.allclose(st_sum[:, 1], (o32 * o32).sum(0), rtol=1e-4)
        outs.append((out.clone(), stats.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # what it does not apply to is refused: data gradients, residual / accumulate epilogues
    d.transposed = 1
    assert l.mbx_conv_supported(C.byref(d)) == -2


@pytest.mark.parametrize("g", [("e1", 3, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)), ("e7", 2, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)),
                               ("e3", 2, 35, 35, 64, 96, 3, 3, 1, (1, 1, 1, 1)),
                               # more tiles than CUs (308 of 128x64, 2.4 per workgroup of 128x128 ...): the queue really hands tiles out
                               ("e4", 16, 35, 35, 64, 320, 1, 1, 1, (0, 0, 0, 0)),
                               # K loops exactly as long as the ring is deep (nk == NST: 3 for the 192x128 / 256x128 tiles, 4 for
                               # the others) with several tiles per workgroup -- the shapes of the detect leg at BATCH_SIZE 256 on
                               # which the queued hand-off of round 3 raced (the loaders read the next tile id one barrier early);
                               # such launches now deal their tiles statically even when a counter is given
                               ("e5", 16, 35, 35, 192, 208, 1, 1, 1, (0, 0, 0, 0)), ("e6", 16, 35, 35, 256, 64, 1, 1, 1, (0, 0, 0, 0))],
                         ids=["1x1", "1x7", "3x3", "1x1_many_tiles", "nk3", "nk4"])
def test_igemm5_epilogues_bit_identical(T, g):
    """Every epilogue of the persistent igemm5 launch (statistics, frozen-BN affine, residual, accumulate + ReLU mask,
    plain scaled store) against the igemm3 launch of the same descriptor: same arithmetic in the same order."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=21)
    gen = torch.Generator().manual_seed(22)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    xb = ops.View.alloc(N, H, W, Ci + 8).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    sc, sh = (torch.rand(Co, generator=gen) + 0.5).cuda(), torch.randn(Co, generator=gen).cuda()
    skip = ops.View.alloc(N, Ho, Wo, Co + 8).slice(8, Co)
    skip.tensor().copy_(torch.randn(N, Ho, Wo, Co, generator=gen).to(torch.bfloat16))
    old = ops.View.alloc(N, Ho, Wo, Co)
    old.tensor().copy_(torch.randn(N, Ho, Wo, Co, generator=gen).to(torch.bfloat16))
    stream = torch.cuda.current_stream().cuda_stream

    def variants(y, stats):
        return {
            "stats": ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y, stats=stats),
            "affine": ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y, epilogue=ops.EPI_AFFINE, relu=1, scale=sc, shift=sh),
            "residual": ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y, epilogue=ops.EPI_RESIDUAL, relu=1, shift=sh, skip=skip, rscale=0.17),
            "acc_mask": ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y, accumulate=1, skip=skip, acc_src=old, rscale=0.2),
            "scaled": ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y, rscale=0.3),
        }
    y0, y1 = ops.View.alloc(N, Ho, Wo, Co, zero=True), ops.View.alloc(N, Ho, Wo, Co, zero=True)
    for cfg in ops.I5_TILE_CONFIGS:
        for kind in ("stats", "affine", "residual", "acc_mask", "scaled"):
            d0 = variants(y0, None)[kind]
            rows0 = ops.conv_stats_rows(d0)
            st0 = torch.zeros((rows0, Co, 2), device="cuda")
            d0 = variants(y0, st0)[kind]
            d1 = variants(y1, None)[kind]
            d1.tile_config = cfg
            rows1 = ops.conv_stats_rows(d1)
            st1 = torch.zeros((rows1, Co, 2), device="cuda")
            d1 = variants(y1, st1)[kind]
            d1.tile_config = cfg
            y0.tensor().zero_(); y1.tensor().zero_()
            if l.mbx_conv_supported(C.byref(d1)) == -2:
                # the tiles with 96 / 64 x 4 channels per wave have no accumulate + mask instantiation (registers)
                assert cfg >= 38 and kind == "acc_mask", (cfg, kind)
                continue
            assert l.mbx_conv(C.byref(d0), stream) == 0 and l.mbx_conv(C.byref(d1), stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(y0.tensor(), y1.tensor()), "%s %s cfg %d" % (name, kind, cfg)
            if kind == "stats":      # partial rows differ with the tile height; their totals are sums of the same bf16 values
                a, b = st0.double().sum(0), st1.double().sum(0)
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-3), "%s stats cfg %d" % (name, cfg)
            # QUEUED tile assignment (mbx_conv_desc.work_counter, a zeroed device int32): the same tiles pulled from a counter
            # instead of dealt statically -- identical output AND identical statistics partials; the launch leaves the
            # counter advanced by the tiles it handed out plus one failed fetch per workgroup lane that ran dry
            ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
            y2 = ops.View.alloc(N, Ho, Wo, Co, zero=True)
            st2 = torch.zeros((rows1, Co, 2), device="cuda")
            d2 = variants(y2, st2)[kind]
            d2.tile_config = cfg
            d2.work_counter = ctr.data_ptr()
            assert l.mbx_conv(C.byref(d2), stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(y1.tensor(), y2.tensor()), "%s %s cfg %d queued" % (name, kind, cfg)
            if kind == "stats":
                assert torch.equal(st1, st2), "%s stats cfg %d queued" % (name, cfg)
            # ... and with a CAPPED grid (mbx_conv_desc.max_workgroups: CUs left to a kernel on another stream), so that
            # every workgroup walks many tiles, queued and statically dealt
            for ctr_on in (True, False):
                ctr.zero_()
                y2.tensor().zero_(); st2.zero_()
                d2.max_workgroups = 24
                d2.work_counter = ctr.data_ptr() if ctr_on else None
                assert l.mbx_conv(C.byref(d2), stream) == 0
                torch.cuda.synchronize()
                assert torch.equal(y1.tensor(), y2.tensor()), "%s %s cfg %d capped queued=%s" % (name, kind, cfg, ctr_on)
                if kind == "stats":
                    assert torch.equal(st1, st2), "%s stats cfg %d capped queued=%s" % (name, cfg, ctr_on)


@pytest.mark.parametrize("g", [("b1", 3, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)), ("b2", 4, 35, 35, 128, 320, 1, 1, 1, (0, 0, 0, 0)),
                               ("b3", 5, 8, 8, 448, 2080, 1, 1, 1, (0, 0, 0, 0)), ("b4", 2, 17, 17, 96, 72, 3, 3, 1, (1, 1, 1, 1))],
                         ids=["block17_up", "block35_up", "block8_up", "3x3_cout72"])
def test_conv_relu_sign_bits(T, g):
    """mbx_conv_desc.relu_bits (round 4).  WRITE: the residual + relu launch stores, beside y, one bit per element = (y > 0),
    eight channels to a byte, 32 channels to a 4-byte store, in a [M, ld_bits] table wider than 4 ceil(C_out / 32) (zeros for
    the channels past C_out, bytes outside untouched) -- y itself is bit-identical to the launch without the table.  READ: the accumulate (+ scale) launch masked by those bits equals,
    bit for bit, the same launch masked by the bf16 tensor (`skip`).  Every tile family: the library's pick and the other
    igemm3 tiles, the persistent igemm5 tiles (EV 7), the panel-resident launch where it applies.  Refusals: with
    statistics, with a `skip` mask as well, on the stride-2 data gradient, on the direct and split-K launches."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=31)
    gen = torch.Generator().manual_seed(32)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    M = N * Ho * Wo
    xb = ops.View.alloc(N, H, W, Ci + 8).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    sh = torch.randn(Co, generator=gen).cuda()
    skip = ops.View.alloc(N, Ho, Wo, Co + 8).slice(8, Co)
    skip.tensor().copy_(torch.randn(N, Ho, Wo, Co, generator=gen).to(torch.bfloat16))
    old = ops.View.alloc(N, Ho, Wo, Co)
    old.tensor().copy_(torch.randn(N, Ho, Wo, Co, generator=gen).to(torch.bfloat16))
    stream = torch.cuda.current_stream().cuda_stream
    wb = (Co + 31) // 32 * 4                    # bytes per pixel row the launch writes
    ldb = wb + 4
    cfgs = [0] + list(range(1, ops.N_TILE_CONFIGS + 1)) + list(ops.I5_TILE_CONFIGS) + [ops.I7_TILE_CONFIG]
    # the block output with exact zeros, negative zeros and tiny values in it: relu(skip + 0.17 (conv + shift))
    y_ref = ops.View.alloc(N, Ho, Wo, Co, zero=True)
    ops.conv(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y_ref, epilogue=ops.EPI_RESIDUAL, relu=1, shift=sh, skip=skip, rscale=0.17))
    torch.cuda.synchronize()
    pos = (y_ref.tensor().float() > 0).reshape(M, Co // 8, 8).to(torch.uint8)
    want = torch.zeros((M, wb), dtype=torch.uint8, device="cuda")
    want[:, :Co // 8] = (pos << torch.arange(8, device="cuda", dtype=torch.uint8)).sum(-1).to(torch.uint8)
    assert 0.2 < float(pos.float().mean()) < 0.8
    ran_w = ran_r = 0
    for cfg in cfgs:
        # ---- write
        bits = torch.full((M, ldb), 0xA5, dtype=torch.uint8, device="cuda")
        y1 = ops.View.alloc(N, Ho, Wo, Co, zero=True)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y1, epilogue=ops.EPI_RESIDUAL, relu=1, shift=sh, skip=skip, rscale=0.17,
                          relu_bits=bits)
        d.tile_config = cfg
        if l.mbx_conv_supported(C.byref(d)) == 0:
            assert l.mbx_conv(C.byref(d), stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(y1.tensor(), y_ref.tensor()), "%s write cfg %d: y" % (name, cfg)
            assert torch.equal(bits[:, :wb], want), "%s write cfg %d: bits" % (name, cfg)
            assert bool((bits[:, wb:] == 0xA5).all()), "%s write cfg %d: bytes outside" % (name, cfg)
            ran_w += 1
        else:
            d.relu_bits = None
            assert l.mbx_conv_supported(C.byref(d)) != 0, "cfg %d refuses the table only" % cfg    # (the tile does not apply at all)
        # ---- read: y = (old + 0.2 conv) masked
        bits = torch.zeros((M, ldb), dtype=torch.uint8, device="cuda")
        bits[:, :wb] = want
        outs = []
        for form in ("skip", "bits"):
            y2 = ops.View.alloc(N, Ho, Wo, Co, zero=True)
            if form == "skip":
                d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y2, accumulate=1, skip=y_ref, acc_src=old, rscale=0.2)
            else:
                d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y2, accumulate=1, acc_src=old, rscale=0.2, relu_bits=bits)
            d.tile_config = cfg if form == "bits" else 0
            if l.mbx_conv_supported(C.byref(d)) != 0:
                outs = None
                break
            assert l.mbx_conv(C.byref(d), stream) == 0
            torch.cuda.synchronize()
            outs.append(y2.tensor().clone())
        if outs is not None:
            assert torch.equal(outs[0], outs[1]), "%s read cfg %d" % (name, cfg)
            ran_r += 1
    assert ran_w >= 8 and ran_r >= 8, (ran_w, ran_r)
    # the mask without an accumulate source, unscaled
    y3, y4 = ops.View.alloc(N, Ho, Wo, Co, zero=True), ops.View.alloc(N, Ho, Wo, Co, zero=True)
    ops.conv(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y3, skip=y_ref))
    ops.conv(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y4, relu_bits=bits))
    torch.cuda.synchronize()
    assert torch.equal(y3.tensor(), y4.tensor())
    # refusals
    stats = torch.zeros((4096, Co, 2), device="cuda")
    assert l.mbx_conv_supported(C.byref(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y3, stats=stats, relu_bits=bits))) != 0
    assert l.mbx_conv_supported(C.byref(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y3, skip=y_ref, relu_bits=bits))) != 0
    assert l.mbx_conv_supported(C.byref(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y3, epilogue=ops.EPI_RESIDUAL, relu=0, shift=sh,
                                                      skip=skip, rscale=0.17, relu_bits=bits))) != 0
    assert l.mbx_conv_supported(C.byref(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y3, epilogue=ops.EPI_AFFINE, relu=1, scale=sh,
                                                      shift=sh, relu_bits=bits))) != 0
    small = torch.zeros((M, wb - 4), dtype=torch.uint8, device="cuda")
    assert l.mbx_conv_supported(C.byref(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y3, relu_bits=small))) != 0
    for bad in (ops.DIRECT3_TILE_CONFIG, ops.DIRECTW_TILE_CONFIG, ops.SPLITK_FLAG + 4):
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], y3, relu_bits=bits)
        d.tile_config = bad
        assert l.mbx_conv_supported(C.byref(d)) != 0, bad


@pytest.mark.parametrize("g", [("p1", 3, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)), ("p2", 4, 35, 35, 128, 320, 1, 1, 1, (0, 0, 0, 0)),
                               ("p3", 16, 17, 17, 320, 1088, 1, 1, 1, (0, 0, 0, 0)), ("p4", 5, 35, 35, 96, 320, 1, 1, 1, (0, 0, 0, 0)),
                               ("p5", 64, 8, 8, 384, 2080, 1, 1, 1, (0, 0, 0, 0))], ids=["k384", "k128", "k320_many_tiles", "k96", "k384_n2080"])
def test_igemm7_panel_resident_bit_identical(T, g):
    """The persistent pointwise launch with the filter panel resident in LDS (tile_config 65, csrc/conv7.hip) against the
    igemm3 launch of the same descriptor, every epilogue it supports (affine, residual, accumulate + ReLU mask, scaled
    store), statically dealt and with work counters: same arithmetic in the same order -> bit-identical."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=31)
    gen = torch.Generator().manual_seed(32)
    xb = ops.View.alloc(N, H, W, Ci + 8).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    sc, sh = (torch.rand(Co, generator=gen) + 0.5).cuda(), torch.randn(Co, generator=gen).cuda()
    skip = ops.View.alloc(N, H, W, Co + 8).slice(8, Co)
    skip.tensor().copy_(torch.randn(N, H, W, Co, generator=gen).to(torch.bfloat16))
    old = ops.View.alloc(N, H, W, Co)
    old.tensor().copy_(torch.randn(N, H, W, Co, generator=gen).to(torch.bfloat16))
    stream = torch.cuda.current_stream().cuda_stream

    def variants(y):
        return {
            "affine": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, epilogue=ops.EPI_AFFINE, relu=1, scale=sc, shift=sh),
            "residual": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, epilogue=ops.EPI_RESIDUAL, relu=1, shift=sh, skip=skip, rscale=0.17),
            "acc_mask": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, accumulate=1, skip=skip, acc_src=old, rscale=0.2),
            "acc_only": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, accumulate=1, acc_src=old),
            "scaled": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, rscale=0.3),
        }
    y0, y1 = ops.View.alloc(N, H, W, Co, zero=True), ops.View.alloc(N, H, W, Co, zero=True)
    for kind in ("affine", "residual", "acc_mask", "acc_only", "scaled"):
        d0 = variants(y0)[kind]
        assert l.mbx_conv(C.byref(d0), stream) == 0
        for queued in (False, True):
            d1 = variants(y1)[kind]
            d1.tile_config = ops.I7_TILE_CONFIG
            ctr = torch.zeros(ops.I7_COUNTERS, dtype=torch.int32, device="cuda")
            if queued:
                d1.work_counter = ctr.data_ptr()
            y1.tensor().zero_()
            assert l.mbx_conv(C.byref(d1), stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(y0.tensor(), y1.tensor()), "%s %s queued=%s" % (name, kind, queued)
    # what it does not apply to is refused, not computed wrongly: statistics epilogue, K > 384, 3x3
    d = ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y1, stats=torch.zeros((ops.conv_stats_rows(variants(y1)["scaled"]) + 8, Co, 2), device="cuda"))
    d.tile_config = ops.I7_TILE_CONFIG
    assert l.mbx_conv(C.byref(d), stream) == -2                      # MBX_ERR_UNSUPPORTED


@pytest.mark.parametrize("g", [("q1", 3, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)), ("q2", 4, 35, 35, 128, 320, 1, 1, 1, (0, 0, 0, 0)),
                               ("q3", 5, 8, 8, 448, 2080, 1, 1, 1, (0, 0, 0, 0)), ("q4", 16, 17, 17, 320, 1088, 1, 1, 1, (0, 0, 0, 0)),
                               ("q5", 5, 35, 35, 96, 320, 1, 1, 1, (0, 0, 0, 0)), ("q6", 64, 8, 8, 384, 2080, 1, 1, 1, (0, 0, 0, 0)),
                               ("q7", 64, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0))],
                         ids=["block17_up", "block35_up", "block8_up", "block17_dgrad_k320", "block35_dgrad_k96", "block8_dgrad_b64", "block17_up_b64"])
def test_conv_pwres_bit_identical(T, g):
    """tile_config 99 (round 5, csrc/convr.hip conv_pwres_kernel): the pointwise launch with an 80-pixel tile resident in LDS and
    the filter streamed per 128 output channels, against the implicit-GEMM launch of the same descriptor: residual + relu with
    and without the sign-bit table (y AND the bits identical), accumulate + tensor mask, accumulate + sign-bit mask, accumulate
    only, scaled -- the block35 / block17 / block8 "up" convolutions (model.py:19-23, 39-43, 59-63) and the data gradients of
    their fused first 1x1s; ragged pixel tiles, column splits (few pixels), more units than workgroups.  Bit-identical."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=41)
    gen = torch.Generator().manual_seed(42)
    M = N * H * W
    xb = ops.View.alloc(N, H, W, Ci + 8).slice(8, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).cuda().contiguous()
    sh = torch.randn(Co, generator=gen).cuda()
    skip = ops.View.alloc(N, H, W, Co + 8).slice(8, Co)
    skip.tensor().copy_(torch.randn(N, H, W, Co, generator=gen).to(torch.bfloat16))
    old = ops.View.alloc(N, H, W, Co)
    old.tensor().copy_(torch.randn(N, H, W, Co, generator=gen).to(torch.bfloat16))
    stream = torch.cuda.current_stream().cuda_stream
    wb = (Co + 31) // 32 * 4
    ldb = wb + 4

    def variants(y, bits):
        return {
            "residual": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, epilogue=ops.EPI_RESIDUAL, relu=1, shift=sh, skip=skip, rscale=0.17),
            "residual_bits": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, epilogue=ops.EPI_RESIDUAL, relu=1, shift=sh, skip=skip, rscale=0.17, relu_bits=bits),
            "residual_norelu": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, epilogue=ops.EPI_RESIDUAL, relu=0, shift=sh, skip=skip, rscale=1.0),
            "acc_mask": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, accumulate=1, skip=skip, acc_src=old, rscale=0.2),
            "acc_bits": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, accumulate=1, acc_src=old, relu_bits=bits),
            "acc_only": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, accumulate=1, acc_src=old),
            "mask_only": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, skip=skip),
            "bits_only": ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, relu_bits=bits, rscale=0.3),
        }
    gbits = torch.randint(0, 256, (M, ldb), dtype=torch.uint8, generator=gen).cuda()
    for kind in ("residual", "residual_bits", "residual_norelu", "acc_mask", "acc_bits", "acc_only", "mask_only", "bits_only"):
        res = []
        for cfg in (0, ops.PWRES_TILE_CONFIG):
            y = ops.View.alloc(N, H, W, Co + 16, zero=True).slice(8, Co)
            bits = torch.full((M, ldb), 0xA5, dtype=torch.uint8, device="cuda") if kind == "residual_bits" else gbits.clone()
            d = variants(y, bits)[kind]
            d.tile_config = cfg
            if cfg and kind in ("acc_mask", "acc_only", "mask_only"):
                assert l.mbx_conv_supported(C.byref(d)) == -2, (kind, cfg)      # (it masks by the sign bits only)
                res.append(res[0])
                continue
            assert l.mbx_conv_supported(C.byref(d)) == 0, (kind, cfg)
            assert l.mbx_conv(C.byref(d), stream) == 0
            torch.cuda.synchronize()
            full = y.buf.reshape(N, H, W, Co + 16)
            assert float(full[..., :8].abs().max()) == 0 and float(full[..., 8 + Co:].abs().max()) == 0
            res.append((y.tensor().clone(), bits.clone()))
        assert torch.equal(res[0][0], res[1][0]), "%s %s: %g" % (name, kind, float((res[0][0].float() - res[1][0].float()).abs().max()))
        assert torch.equal(res[0][1], res[1][1]), "%s %s: bits" % (name, kind)
        assert float(res[1][0].float().abs().max()) > 0
    # what it does not apply to is refused: statistics, a plain store, 3x3
    y = ops.View.alloc(N, H, W, Co, zero=True)
    d = ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y)
    d.tile_config = ops.PWRES_TILE_CONFIG
    assert l.mbx_conv_supported(C.byref(d)) == -2
    d = ops.make_desc(xb, wd, Co, 1, 1, 1, 0, 0, y, stats=torch.zeros((M, Co, 2), device="cuda"))
    d.tile_config = ops.PWRES_TILE_CONFIG
    assert l.mbx_conv_supported(C.byref(d)) == -2


def test_conv_f32_head_output(T):
    """model.py:213-219: 1x1, no BN/bias/act, C_out = 5k = 25 (locations 4k + confidences k), fp32 out."""
    torch = T
    from multibox_amd import ops
    g = ("h", 3, 6, 6, 96, 25, 1, 1, 1, (0, 0, 0, 0))
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=5)
    ref = ref_conv(torch, x, w, st, pads)
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    y = ops.View.alloc(N, H, W, Co, ld=32, dtype=torch.float32, zero=True)
    ops.conv(ops.make_desc(xb, w.to(torch.bfloat16).cuda(), Co, R, S, st, 0, 0, y, epilogue=ops.EPI_STORE_F32))
    ok, msg = close(torch, y.tensor(), ref, f32=True)
    assert ok, msg
    assert float(y.buf.reshape(N, H, W, 32)[..., Co:].abs().max()) == 0


@pytest.mark.parametrize("g", GEOMS[:12], ids=[g[0] for g in GEOMS[:12]])
def test_conv_dgrad_wgrad(T, g):
    torch = T
    from multibox_amd import ops
    name, N, H, W, Ci, Co, R, S, st, pads = g
    x, w = make_case(torch, g, seed=7)
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    gen = torch.Generator().manual_seed(8)
    dy = bf16_round(torch, torch.randn(N, Ho, Wo, Co, generator=gen))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref_conv(torch, xr, wr, st, pads).backward(dy)
    dyb = ops.View.alloc(N, Ho, Wo, Co + 8).slice(8, Co)
    dyb.buf.zero_()
    dyb.tensor().copy_(dy.to(torch.bfloat16))
    # ---- data gradient: transposed conv with the flipped, channel-transposed filter
    wT = w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(torch.bfloat16).cuda()       # [Ci][R][S][Co]
    dx = ops.View.alloc(N, H, W, Ci + 8, zero=True).slice(0, Ci)
    ops.conv(ops.make_desc(dyb, wT, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], dx, transposed=1))
    ok, msg = close(torch, dx.tensor(), xr.grad)
    assert ok, "dgrad: " + msg
    # ---- weight (+ bias) gradient
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    dw = torch.zeros((Co, R, S, Ci), dtype=torch.float32, device="cuda")
    db = torch.zeros((Co,), dtype=torch.float32, device="cuda")
    yv = ops.View.alloc(N, Ho, Wo, Co)
    d = ops.make_desc(xb, None, Co, R, S, st, pads[0], pads[1], yv)
    ops.conv_wgrad(d, dyb, dw, db)
    ok, msg = close(torch, dw, wr.grad, f32=True)
    assert ok, "wgrad: " + msg
    ok, msg = close(torch, db, dy.reshape(-1, Co).sum(0), f32=True)
    assert ok, "bias grad: " + msg
    # every selectable block shape / split count (mbx_conv_desc.tile_config 1..10; 7..10 are the narrow tile) gives the same sums
    for cfg in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10):
        d.tile_config = cfg
        dw.zero_(); db.zero_()
        ops.conv_wgrad(d, dyb, dw, db)
        ok, msg = close(torch, dw, wr.grad, f32=True)
        assert ok, "wgrad tile_config %d: %s" % (cfg, msg)
        ok, msg = close(torch, db, dy.reshape(-1, Co).sum(0), f32=True)
        assert ok, "bias grad tile_config %d: %s" % (cfg, msg)
    d.tile_config = 0
    # ... and so does every igemm tile configuration, forward and data gradient (same K order: bit-identical outputs)
    yv2 = ops.View.alloc(N, Ho, Wo, Co)
    wdev = w.to(torch.bfloat16).cuda().contiguous()             # keep it alive: the descriptor holds a raw pointer
    dfw = ops.make_desc(xb, wdev, Co, R, S, st, pads[0], pads[1], yv)
    ops.conv(dfw)
    ddg = ops.make_desc(dyb, wT, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], dx, transposed=1)
    dx_ref = dx.tensor().clone()
    for cfg in range(1, ops.N_TILE_CONFIGS + 1):
        dfw.tile_config = cfg
        dfw.y = yv2.ptr
        ops.conv(dfw)
        assert torch.equal(yv2.tensor(), yv.tensor()), "forward tile_config %d" % cfg
        ddg.tile_config = cfg
        dx.tensor().zero_()
        ops.conv(ddg)
        assert torch.equal(dx.tensor(), dx_ref), "dgrad tile_config %d" % cfg
    # ... and the persistent igemm5 launches (tile_config 32 + t: 8 MFMA waves + 8 loader waves, tiles walked by one block
    # per CU): same K order and MFMA order, so bit-identical too; the stride-2 data gradient stays on igemm3 (-2)
    import ctypes as C
    from multibox_amd import _lib
    l = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    for cfg in ops.I5_TILE_CONFIGS:
        dfw.tile_config = cfg
        yv2.tensor().zero_()
        assert l.mbx_conv(C.byref(dfw), stream) == 0
        assert torch.equal(yv2.tensor(), yv.tensor()), "forward igemm5 tile_config %d" % cfg
        ddg.tile_config = cfg
        dx.tensor().zero_()
        rc = l.mbx_conv(C.byref(ddg), stream)
        assert rc == (0 if st == 1 else -2), (cfg, rc)
        if rc == 0:
            assert torch.equal(dx.tensor(), dx_ref), "dgrad igemm5 tile_config %d" % cfg


def test_wgrad_odd_cout_padded_dy(T):
    """Head output conv: C_out = 25 with dy padded to ld 32 (zeros beyond 25)."""
    torch = T
    from multibox_amd import ops
    N, H, W, Ci, Co = 4, 6, 6, 96, 25
    gen = torch.Generator().manual_seed(9)
    x = bf16_round(torch, torch.randn(N, H, W, Ci, generator=gen))
    dy = bf16_round(torch, torch.randn(N, H, W, Co, generator=gen))
    ref = torch.einsum("nhwk,nhwc->kc", dy, x).reshape(Co, 1, 1, Ci)
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    dyb = ops.View.alloc(N, H, W, Co, ld=32, zero=True)
    dyb.tensor().copy_(dy.to(torch.bfloat16))
    dw = torch.zeros((Co, 1, 1, Ci), dtype=torch.float32, device="cuda")
    d = ops.make_desc(xb, None, Co, 1, 1, 1, 0, 0, ops.View.alloc(N, H, W, 32))
    d.C_out = Co
    ops.conv_wgrad(d, dyb, dw)
    ok, msg = close(torch, dw, ref, f32=True)
    assert ok, msg


# BASELINE config (ii) layer shapes at the full BATCH_SIZE = 64: pixel counts that are not multiples of any tile
# (18496, 78400), every kernel mode (pointwise, general, stride-2 data gradient with tap skipping), all tile configs.
FULL = [
    ("b17_fused_1x1_1088_320", 17, 17, 1088, 320, 1, 1, 1, (0, 0, 0, 0)),
    ("b17_up_1x1_384_1088", 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)),
    ("b17_1x7_128_160", 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)),
    ("b35_3x3_48_64", 35, 35, 48, 64, 3, 3, 1, (1, 1, 1, 1)),
    ("b35_fused_1x1_320_96", 35, 35, 320, 96, 1, 1, 1, (0, 0, 0, 0)),
    ("m6a_3x3_s2_320_384", 35, 35, 320, 384, 3, 3, 2, (0, 0, 0, 0)),
    ("m7a_3x3_s2_256_288", 17, 17, 256, 288, 3, 3, 2, (0, 0, 0, 0)),
    ("head_3x3_s2_same_1536_256", 8, 8, 1536, 256, 3, 3, 2, (0, 0, 1, 1)),
]


@pytest.mark.parametrize("g", FULL, ids=[g[0] for g in FULL])
def test_conv_full_size_b64(T, g):
    """Forward, data gradient and weight gradient at BATCH_SIZE 64 against a float32 reference computed ON THE GPU
    from plain torch ops (unfold + matmul + autograd; no kernel of this library), same bf16-rounded inputs."""
    torch = T
    import torch.nn.functional as F
    from multibox_amd import ops
    name, H, W, Ci, Co, R, S, st, pads = g
    N = 64
    gen = torch.Generator().manual_seed(11)
    x = bf16_round(torch, torch.randn(N, H, W, Ci, generator=gen)).cuda()
    w = bf16_round(torch, torch.randn(Co, R, S, Ci, generator=gen) / (R * S * Ci) ** 0.5).cuda()
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    dy = bf16_round(torch, torch.randn(N, Ho, Wo, Co, generator=gen)).cuda()
    torch.backends.cuda.matmul.allow_tf32 = False
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xp = F.pad(xr.permute(0, 3, 1, 2), (pads[1], pads[3], pads[0], pads[2]))
    cols = F.unfold(xp, (R, S), stride=st)                                   # [N, Ci*R*S, Ho*Wo], channel-major patches
    wm = wr.permute(0, 3, 1, 2).reshape(Co, Ci * R * S)
    ref = (cols.transpose(1, 2) @ wm.t()).reshape(N, Ho, Wo, Co)
    ref.backward(dy)
    xb, yb = ops.View.alloc(N, H, W, Ci), ops.View.alloc(N, Ho, Wo, Co)
    xb.tensor().copy_(x.to(torch.bfloat16))
    wd = w.to(torch.bfloat16).contiguous()
    ops.conv(ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb))
    ok, msg = close(torch, yb.tensor(), ref.detach())
    assert ok, "forward: " + msg
    dyb = ops.View.alloc(N, Ho, Wo, Co)
    dyb.tensor().copy_(dy.to(torch.bfloat16))
    wT = w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(torch.bfloat16)
    dx = ops.View.alloc(N, H, W, Ci, zero=True)
    ops.conv(ops.make_desc(dyb, wT, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], dx, transposed=1))
    ok, msg = close(torch, dx.tensor(), xr.grad)
    assert ok, "dgrad: " + msg
    dw = torch.zeros((Co, R, S, Ci), dtype=torch.float32, device="cuda")
    ops.conv_wgrad(ops.make_desc(xb, None, Co, R, S, st, pads[0], pads[1], yb), dyb, dw)
    ok, msg = close(torch, dw, wr.grad, f32=True)
    assert ok, "wgrad: " + msg


@pytest.mark.parametrize("deterministic", [False, True])
def test_wgrad_grouped_matches_reference_and_single_layer_api(T, deterministic):
    """mbx_conv_wgrad_grouped: the weight gradients of MANY layers in one launch (every geometry above + a 25-channel
    head with padded dy + scaled jobs with a bias) against the float32 torch reference; the deterministic plan
    (no split pixel reductions) must give bit-identical results on a second launch."""
    torch = T
    import torch.nn.functional as F
    from multibox_amd import ops
    jobs, checks, keep = [], [], []
    geoms = [g for g in GEOMS if g[0] != "1x1_2080_1536_m4096"] + [("head_25", 4, 6, 6, 96, 25, 1, 1, 1, (0, 0, 0, 0))]
    for i, g in enumerate(geoms):
        name, N, H, W, Ci, Co, R, S, st, pads = g
        gen = torch.Generator().manual_seed(100 + i)
        x = bf16_round(torch, torch.randn(N, H, W, Ci, generator=gen))
        Ho, Wo = out_hw(H, W, R, S, st, pads)
        dy = bf16_round(torch, torch.randn(N, Ho, Wo, Co, generator=gen))
        scale = 1.0 if i % 3 else 0.17
        use_bias = (i % 3 == 0)
        wr = torch.zeros(Co, R, S, Ci, requires_grad=True)
        xt = F.pad(x.permute(0, 3, 1, 2), (pads[1], pads[3], pads[0], pads[2]))
        y = F.conv2d(xt, wr.permute(0, 3, 1, 2), stride=st).permute(0, 2, 3, 1)
        (y * dy).sum().backward()
        xb = ops.View.alloc(N, H, W, Ci + 8, zero=True).slice(8, Ci) if i % 2 else ops.View.alloc(N, H, W, Ci)
        xb.tensor().copy_(x.to(torch.bfloat16))
        ld = (Co + 7) // 8 * 8
        dyb = ops.View.alloc(N, Ho, Wo, Co, ld=ld, zero=True)
        dyb.tensor().copy_(dy.to(torch.bfloat16))
        dw = torch.zeros((Co, R, S, Ci), dtype=torch.float32, device="cuda")
        db = torch.zeros((Co,), dtype=torch.float32, device="cuda") if use_bias else None
        j = ops.WgradJob()
        j.desc = ops.make_desc(xb, None, Co, R, S, st, pads[0], pads[1], ops.View(dyb.buf, N, Ho, Wo, 8, ld, 0, 2))
        j.desc.C_out = Co
        j.dy, j.dy_img_stride, j.ld_dy, j.scale = dyb.ptr, dyb.img_stride, dyb.ld, scale
        j.dw, j.db = dw.data_ptr(), (None if db is None else db.data_ptr())
        jobs.append(j)
        keep.append((xb, dyb))
        checks.append((name, dw, db, wr.grad * scale, dy.reshape(-1, Co).sum(0) * scale))
    grp = ops.WgradGroup(jobs, deterministic=deterministic)
    assert grp.info.n_layers == len(jobs) and grp.info.n_items >= len(jobs)
    grp.launch()
    torch.cuda.synchronize()
    for name, dw, db, ref_w, ref_b in checks:
        ok, msg = close(torch, dw, ref_w, f32=True)
        assert ok, "grouped wgrad %s: %s" % (name, msg)
        if db is not None:
            ok, msg = close(torch, db, ref_b, f32=True)
            assert ok, "grouped bias grad %s: %s" % (name, msg)
    if deterministic:
        first = [(dw.clone(), None if db is None else db.clone()) for _, dw, db, _, _ in checks]
        for _, dw, db, _, _ in checks:
            dw.zero_()
            if db is not None:
                db.zero_()
        grp.launch()
        torch.cuda.synchronize()
        for (name, dw, db, _, _), (dw0, db0) in zip(checks, first):
            assert torch.equal(dw, dw0), "deterministic plan not bit-reproducible: " + name
            assert db is None or torch.equal(db, db0)
        # a CAPPED grid (mbx_conv_wgrad_grouped_capped: 24 persistent workgroups drain the same queues) gives the same bits
        for _, dw, db, _, _ in checks:
            dw.zero_()
            if db is not None:
                db.zero_()
        grp.launch(max_workgroups=24)
        torch.cuda.synchronize()
        for (name, dw, db, _, _), (dw0, db0) in zip(checks, first):
            assert torch.equal(dw, dw0), "capped launch differs: " + name
            assert db is None or torch.equal(db, db0)
        assert grp.completed_ok()


FUSED_APPLY_CASES = [
    # (geometry, tile_config, max_workgroups): igemm5 tiles on block35 / block17 / block8 / Mixed shapes; ragged M and C_out; several
    # tiles per workgroup (capped grids: the tail walks every tile the workgroup stored); the output a channel slice of a wider buffer
    (("f17", 64, 17, 17, 1088, 320, 1, 1, 1, (0, 0, 0, 0)), 36, 0),
    (("f17cap", 64, 17, 17, 1088, 320, 1, 1, 1, (0, 0, 0, 0)), 36, 48),
    (("f35", 64, 35, 35, 320, 96, 1, 1, 1, (0, 0, 0, 0)), 35, 0),
    (("f8", 64, 8, 8, 2080, 384, 1, 1, 1, (0, 0, 0, 0)), 34, 0),
    (("f3x3", 5, 35, 35, 256, 256, 3, 3, 1, (1, 1, 1, 1)), 36, 0),
    (("fragged", 3, 17, 17, 256, 200, 3, 3, 1, (1, 1, 1, 1)), 33, 7),
    (("f7b", 8, 8, 8, 2080, 1536, 1, 1, 1, (0, 0, 0, 0)), 34, 0),
    (("fw", 64, 35, 35, 48, 64, 3, 3, 1, (1, 1, 1, 1)), 97, 0),
    (("fw2", 7, 35, 35, 32, 48, 3, 3, 1, (1, 1, 1, 1)), 97, 0),
    (("fr17a", 64, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), 98, 0),
    (("fr17b", 64, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)), 98, 0),
    (("fr17cap", 40, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)), 98, 50),
    (("fr8", 64, 8, 8, 192, 224, 1, 3, 1, (0, 1, 0, 1)), 98, 0),
    (("fr8b", 64, 8, 8, 224, 256, 3, 1, 1, (1, 0, 1, 0)), 98, 0),
]


@pytest.mark.parametrize("case", FUSED_APPLY_CASES, ids=[c[0][0] for c in FUSED_APPLY_CASES])
@pytest.mark.parametrize("relu", [1, 0])
def test_conv_fused_bn_apply_bit_identical(T, case, relu):
    """Round 6: mbx_conv_desc.bn_apply -- the layer's BN apply as the TAIL of the convolution launch behind a
    one-shot grid barrier (csrc/fused_bn.h) -- against the two launches it replaces (the same convolution, then
    mbx_bn_apply_fused_mapped on the rows it added): y, the activation, mean, rstd, the relu threshold and the stored batch
    variance are the SAME BITS; the moving-average form (decay >= 0) too; slices of wider buffers untouched outside; the barrier
    did not time out (flag word 1 of the control block stays 0, the step control word stays 0)."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    g, cfg, cap = case
    name, N, H, W, Ci, Co, R, S, st, pads = g
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    M = N * Ho * Wo
    stream = torch.cuda.current_stream().cuda_stream
    x, w = make_case(torch, g, seed=7)
    wd = w.to(torch.bfloat16).cuda().contiguous()
    gen = torch.Generator().manual_seed(9)
    beta = (torch.randn(Co, generator=gen) * 0.3).cuda()
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(x.to(torch.bfloat16))
    res = []
    for fused in (False, True):
        for decay in (-1.0, 0.9):
            yb = ops.View.alloc(N, Ho, Wo, Co, zero=True)
            a = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
            table = torch.zeros((8, Co, 2), dtype=torch.int64, device="cuda")
            mean, rstd, thr = torch.zeros(Co, device="cuda"), torch.zeros(Co, device="cuda"), torch.zeros(Co, device="cuda")
            mm, mv = torch.full((Co,), 0.25, device="cuda"), torch.full((Co,), 1.5, device="cuda")
            bar = torch.zeros(ops.GRID_BARRIER_BYTES // 4 + 32, dtype=torch.int32, device="cuda")
            boff = (-(bar.data_ptr() // 4)) % 32
            ctl = torch.zeros(8, device="cuda")
            d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=table, stats_rows_mod=8, stats_ld=Co)
            d.tile_config, d.max_workgroups = cfg, cap
            if fused:
                ba = ops.BnApplyDesc()
                ba.barrier = bar.data_ptr() + 4 * boff
                ba.a, ba.ld_a, ba.beta, ba.mean, ba.rstd = a.ptr, a.ld, beta.data_ptr(), mean.data_ptr(), rstd.data_ptr()
                ba.moving_mean, ba.moving_var, ba.relu_thr = mm.data_ptr(), mv.data_ptr(), thr.data_ptr()
                ba.relu, ba.eps, ba.decay, ba.step_poison = relu, 0.001, decay, ctl.data_ptr()
                d.bn_apply = C.addressof(ba)
                assert l.mbx_conv_supported(C.byref(d)) == 0
                ops.conv(d)
                torch.cuda.synchronize()
                assert int(bar[boff + 1]) == 0 and float(ctl[0]) == 0.0, "grid barrier timed out"
                assert int(bar[boff]) > 0                                    # (workgroup 0 recorded the grid size: the tail ran)
            else:
                assert l.mbx_conv_supported(C.byref(d)) == 0
                ops.conv(d)
                assert l.mbx_bn_apply_fused_mapped(table.data_ptr(), 8, M, 0.001, decay, yb.ptr, M, Co, beta.data_ptr(), relu, a.ptr, a.ld,
                                                   None, mean.data_ptr(), rstd.data_ptr(), mm.data_ptr(), mv.data_ptr(), thr.data_ptr(),
                                                   stream) == 0
                torch.cuda.synchronize()
            res.append((yb.tensor().clone(), a.buf.clone(), mean, rstd, thr, mm, mv, table.clone()))
    for i in range(2):
        s_, f_ = res[i], res[2 + i]
        for k_, nm in enumerate(("y", "a (whole buffer)", "mean", "rstd", "relu_thr", "moving_mean", "moving_var", "rows")):
            assert torch.equal(s_[k_].view(torch.int16 if s_[k_].dtype == torch.bfloat16 else s_[k_].dtype),
                               f_[k_].view(torch.int16 if f_[k_].dtype == torch.bfloat16 else f_[k_].dtype)), (name, nm, i)
    a_full = res[2][1].reshape(N, Ho, Wo, Co + 24)
    assert float(a_full[..., :16].abs().max()) == 0 and float(a_full[..., 16 + Co:].abs().max()) == 0
    assert bool(torch.isfinite(res[2][1].float()).all()) and float(res[2][1].float().abs().max()) > 0


FUSED_BWD_CASES = [
    # (forward geometry of consumer X, tile_config of its data gradient, max_workgroups, channel split of X's INPUT into BN layers)
    # block17 "up" 384 -> 1088: its data gradient writes da of [b0 192 | 7x1 192] = two batch-norm layers; igemm5 256x128
    (("b17up", 64, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)), 36, 0, (192, 192)),
    (("b17upcap", 16, 17, 17, 384, 1088, 1, 1, 1, (0, 0, 0, 0)), 34, 20, (192, 192)),           # several tiles per workgroup
    (("b8up", 64, 8, 8, 448, 2080, 1, 1, 1, (0, 0, 0, 0)), 33, 0, (192, 256)),
    (("b35up", 16, 35, 35, 128, 320, 1, 1, 1, (0, 0, 0, 0)), 35, 0, (32, 32, 64)),
    (("b17_7x1", 64, 17, 17, 160, 192, 7, 1, 1, (3, 0, 3, 0)), 98, 0, (160,)),                    # resident image
    (("b17_1x7", 40, 17, 17, 128, 160, 1, 7, 1, (0, 3, 0, 3)), 98, 0, (128,)),
    (("b8_3x1", 64, 8, 8, 224, 256, 3, 1, 1, (1, 0, 1, 0)), 98, 0, (224,)),
    (("b35_3x3", 20, 35, 35, 48, 64, 3, 3, 1, (1, 1, 1, 1)), 97, 0, (48,)),                        # whole-width direct
    (("b35_3x3b", 64, 35, 35, 32, 32, 3, 3, 1, (1, 1, 1, 1)), 97, 0, (32,)),                       # more tiles than workgroups
    (("m6a", 6, 35, 35, 256, 256, 3, 3, 1, (1, 1, 1, 1)), 34, 0, (256,)),
]


@pytest.mark.parametrize("case", FUSED_BWD_CASES, ids=[c[0][0] for c in FUSED_BWD_CASES])
def test_conv_fused_bn_backward_matches_separate_launches(T, case):
    """Round 6: mbx_conv_desc.bn_bwd -- the batch-norm backward of the layers whose activation gradient a
    data gradient writes, as the TAIL of that data-gradient launch (csrc/fused_bn.h) -- against the launches it replaces: the
    same data gradient, then mbx_bn_bwd_onepass per layer on the da it wrote.  da is the same bits; dy within one bf16 ulp
    (the totals are float sums whose grouping differs: |dy - ref| <= 2^-7 |ref| + 2e-3 max|ref| -- the stated tolerance of
    every bf16 output in this file) and d(beta) to rtol 1e-4; several layers per launch (channel segments of a concat buffer),
    layers with and without relu, capped grids (several tiles per workgroup), the three kernel families."""
    torch = T
    import ctypes as C
    from multibox_amd import ops, _lib
    l = _lib.lib()
    g, cfg, cap, split = case
    name, N, H, W, Ci, Co, R, S, st, pads = g
    assert sum(split) == Ci
    Ho, Wo = out_hw(H, W, R, S, st, pads)
    M = N * H * W                                       # pixels of X's input = rows of da / y / dy of the layers it feeds
    stream = torch.cuda.current_stream().cuda_stream
    x, w = make_case(torch, g, seed=11)
    gen = torch.Generator().manual_seed(12)
    dyX = bf16_round(torch, torch.randn(N, Ho, Wo, Co, generator=gen))
    dyb = ops.View.alloc(N, Ho, Wo, Co)
    dyb.tensor().copy_(dyX.to(torch.bfloat16))
    wT = w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(torch.bfloat16).cuda()       # [Ci][R][S][Co]
    # the layers X's input is made of: pre-BN outputs y (each layer's own [M, K] tensor), statistics, beta; odd layers without relu
    layers = []
    for i, K in enumerate(split):
        y = (torch.randn(M, K, generator=gen) * 1.5 + 0.3).to(torch.bfloat16).cuda()
        yf = y.float()
        mean = yf.mean(0).contiguous()
        rstd = (1.0 / torch.sqrt(yf.var(0, unbiased=False) + 0.001)).contiguous()
        beta = (torch.randn(K, generator=gen) * 0.3).cuda()
        layers.append(dict(K=K, y=y, mean=mean, rstd=rstd, beta=beta, relu=int(i % 2 == 0)))

    def run(fused):
        da = ops.View.alloc(N, H, W, Ci + 16, zero=True).slice(8, Ci)              # a channel slice of a wider gradient buffer
        d = ops.make_desc(dyb, wT, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], da, transposed=1, rscale=(0.17 if R * S == 1 else 0.0))
        d.tile_config, d.max_workgroups = cfg, cap
        outs = [dict(dy=torch.zeros((M, L["K"]), dtype=torch.bfloat16, device="cuda"), dbeta=torch.zeros(L["K"], device="cuda")) for L in layers]
        if fused:
            t = ops.BnBwdFused()
            bar = torch.zeros(ops.GRID_BARRIER_BYTES // 4 + 32, dtype=torch.int32, device="cuda")
            boff = (-(bar.data_ptr() // 4)) % 32
            ctl = torch.zeros(8, device="cuda")
            accs = [torch.zeros((ops.BN_BWD_SLOTS, 2, L["K"]), device="cuda") for L in layers]
            t.barrier, t.n, t.step_poison = bar.data_ptr() + 4 * boff, len(layers), ctl.data_ptr()
            c0 = 0
            for i, (L, o, a) in enumerate(zip(layers, outs, accs)):
                t.c_begin[i] = c0
                t.y[i], t.ld_y[i], t.dy[i], t.ld_dy[i] = L["y"].data_ptr(), L["K"], o["dy"].data_ptr(), L["K"]
                t.mean[i], t.rstd[i], t.beta[i], t.dbeta[i] = L["mean"].data_ptr(), L["rstd"].data_ptr(), L["beta"].data_ptr(), o["dbeta"].data_ptr()
                t.acc[i], t.acc_ld[i], t.relu[i] = a.data_ptr(), L["K"], L["relu"]
                c0 += L["K"]
            d.bn_bwd = C.addressof(t)
            assert l.mbx_conv_supported(C.byref(d)) == 0
            ops.conv(d)
            torch.cuda.synchronize()
            assert int(bar[boff + 1]) == 0 and float(ctl[0]) == 0.0 and int(bar[boff]) > 0, "grid barrier timed out / tail did not run"
        else:
            assert l.mbx_conv_supported(C.byref(d)) == 0
            ops.conv(d)
            c0 = 0
            for L, o in zip(layers, outs):
                K = L["K"]
                assert l.mbx_bn_bwd_onepass_supported(M, K, 0) == 1
                ws = torch.zeros(l.mbx_bn_bwd_onepass_workspace_bytes(K) // 4, device="cuda")
                dav = da.slice(c0, K)
                _lib.check(l.mbx_bn_bwd_onepass(dav.ptr, dav.ld, L["relu"], L["y"].data_ptr(), M, K, L["mean"].data_ptr(), L["rstd"].data_ptr(),
                                                L["beta"].data_ptr(), o["dbeta"].data_ptr(), o["dy"].data_ptr(), ws.data_ptr(), 0, None, stream),
                           "bn_bwd_onepass")
                c0 += K
            torch.cuda.synchronize()
        return da.buf.clone(), outs
    da0, ref = run(False)
    da1, got = run(True)
    assert torch.equal(da0.view(torch.int16), da1.view(torch.int16)), "da differs"
    assert float(da1.float().abs().max()) > 0
    for i, (r, o) in enumerate(zip(ref, got)):
        assert bool(torch.isfinite(o["dy"].float()).all())
        ok, msg = close(torch, o["dy"], r["dy"])
        assert ok, "layer %d dy: %s" % (i, msg)
        assert torch.allclose(o["dbeta"], r["dbeta"], rtol=1e-4, atol=1e-4 * float(r["dbeta"].abs().max())), "layer %d dbeta" % i
