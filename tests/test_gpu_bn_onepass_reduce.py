"""One-launch BN backward: the workgroup's column-parallel reduction in front of the atomics, and the 16-byte read
of the totals behind the grid barrier, on the smallest shapes that reach every path of that reduction.

With C channels a 512-thread workgroup holds rpi = 512 / (C/8) rows per sweep and reduces them as [rpi][2C]:
  2C < 512  : np = 512 / 2C row parts (a second LDS stage when np > 1), ragged when rpi % np != 0
  2C >= 512 : thread t owns columns t, t + 512, ...; the rows/columns per LDS round trip depend on rpi (1, 2, 3-4, 5-8, 9+)

The reference is NOT the project's three-launch kernels but the float64 formula on the host from the same bf16 inputs:
  xh = (y - mean) * rstd, g = da where (no relu or xh + beta > 0) else 0,
  dy = rstd * (g - mean(g) - xh * mean(g * xh)), dbeta += sum(g).
y is generated so that no element has |xh + beta| < 1e-3 (asserted), so a fused-multiply rounding cannot flip a mask
and no element is excluded.  Tolerances are those of test_gpu_nnops.py: dy within one bf16 ulp (2^-7 relative +
2e-3 of max|ref|), dbeta rtol 1e-4 / atol 1e-3 max|ref|; the barrier's time-out flag must be 0.
"""
import functools

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [
    (1225, 64), (1225, 80), (1225, 48), (1225, 96), (1001, 24),      # 2C < 512: np = 4, 3, 5, 2, 10; rpi % np ragged
    (300, 8),                                                        # C/8 = 1: 512 rows per sweep, np = 32
    (289, 320), (130, 1088), (64, 2080),                             # 2C >= 512: rpi = 12, 3, 1; up to 9 columns per thread
    (289, 160), (289, 192), (64, 224), (64, 384),                    # block17 / block8 widths (np = 1 with 2C < 512; rpi = 10)
]
PAD = 16            # da lives in a view [M, C + PAD] at channel offset 8
OFF = 8
SLOTS = 8           # accumulator copies in front of the control words of the workspace
MARGIN = 1e-3


@pytest.fixture(scope="module")
def T():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()
    return torch


def close_bf16(out, ref):
    """test_gpu_nnops.py:27"""
    out, ref = out.float().cpu(), ref.float().cpu()
    mx = float(ref.abs().max()) + 1e-20
    err = (out - ref).abs()
    bad = err > (2.0 ** -7) * ref.abs() + 2e-3 * mx
    return int(bad.sum()) == 0, "%d/%d bad, max err %.3g, max|ref| %.3g" % (int(bad.sum()), bad.numel(), float(err.max()), mx)


@functools.lru_cache(maxsize=None)
def inputs(M, Cc):
    """bf16 y / da, float32 mean / rstd / beta (host tensors), with every |xh + beta| >= MARGIN."""
    import torch
    gen = torch.Generator().manual_seed(M * 131 + Cc)
    beta = torch.randn(Cc, generator=gen) * 0.3
    yf = torch.randn(M, Cc, generator=gen) * 2 + 0.5
    for _ in range(20):
        y = yf.to(torch.bfloat16)
        mean = y.float().mean(0)
        rstd = torch.rsqrt(y.float().var(0, unbiased=False) + 0.001)
        xh = (y.double() - mean.double()) * rstd.double()
        near = (xh + beta.double()).abs() < MARGIN
        if not bool(near.any()):
            break
        yf[near] = (torch.randn(int(near.sum()), generator=gen) * 2 + 0.5)       # regenerate the offenders, before rounding
    da = torch.randn(M, Cc, generator=gen).to(torch.bfloat16)
    prefill = torch.randn(Cc, generator=gen)
    return y, da, mean.contiguous(), rstd.contiguous(), beta.contiguous(), prefill


@functools.lru_cache(maxsize=None)
def reference(M, Cc, relu):
    y, da, mean, rstd, beta, prefill = inputs(M, Cc)
    xh = (y.double() - mean.double()) * rstd.double()
    pre = xh + beta.double()
    assert float(pre.abs().min()) >= MARGIN                # the precondition: no mask can flip on a rounding
    g = da.double() * (pre > 0) if relu else da.double()
    dy = rstd.double() * (g - g.mean(0) - xh * (g * xh).mean(0))
    return dy, prefill.double() + g.sum(0)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("M,Cc", SHAPES)
def test_onepass_reduce(T, M, Cc, relu):
    torch = T
    from multibox_amd import _lib
    l = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    y, da, mean, rstd, beta, prefill = inputs(M, Cc)
    dy_ref, dbeta_ref = reference(M, Cc, relu)
    assert l.mbx_bn_bwd_onepass_supported(M, Cc, 0) == 1
    yd, md, rd, bd = y.cuda(), mean.cuda(), rstd.cuda(), beta.cuda()
    # the gradient in a wider view: NaN in the channels outside it, which must be neither read nor written
    wide = torch.full((M, Cc + PAD), float("nan"), dtype=torch.bfloat16)
    wide[:, OFF:OFF + Cc] = da
    wide_d = wide.cuda()
    da_ptr = wide_d.data_ptr() + OFF * 2
    nws = l.mbx_bn_bwd_onepass_workspace_bytes(Cc) // 4
    ran = 0
    for max_wg in (0, 8):       # all CUs: short slices; 8 workgroups: long slices, more vectors per lane
        if not l.mbx_bn_bwd_onepass_supported(M, Cc, max_wg):
            continue
        ws = torch.zeros(nws, device="cuda")
        dbeta = prefill.cuda()                                                        # the kernel accumulates into it
        dy = torch.full((M + 1, Cc), 7.0, dtype=torch.bfloat16, device="cuda")        # guard row behind dy
        _lib.check(l.mbx_bn_bwd_onepass_mapped(da_ptr, Cc + PAD, relu, yd.data_ptr(), M, Cc, md.data_ptr(), rd.data_ptr(),
                                               bd.data_ptr(), dbeta.data_ptr(), dy.data_ptr(), ws.data_ptr(), max_wg, None,
                                               None, stream))
        torch.cuda.synchronize()
        flags = ws[SLOTS * 2 * Cc:SLOTS * 2 * Cc + 2].view(torch.int32).tolist()
        assert flags[1] == 0, "grid barrier timed out (max_workgroups %d)" % max_wg
        assert 0 < flags[0] <= (max_wg or 1 << 30)
        ok, msg = close_bf16(dy[:M], dy_ref)
        print("M %d C %d relu %d max_wg %d grid %d: dy %s, dbeta max err %.3g" %
              (M, Cc, relu, max_wg, flags[0], msg, float((dbeta.cpu().double() - dbeta_ref).abs().max())))
        assert ok, "dy (max_workgroups %d): %s" % (max_wg, msg)
        assert torch.allclose(dbeta.cpu().double(), dbeta_ref, rtol=1e-4, atol=1e-3 * float(dbeta_ref.abs().max()))
        assert bool((dy[M] == 7.0).all()), "guard row behind dy written"
        got = wide_d.cpu()
        assert torch.equal(got[:, OFF:OFF + Cc], da) and bool(got[:, :OFF].isnan().all()) and bool(got[:, OFF + Cc:].isnan().all())
        ran += 1
    assert ran >= 1
