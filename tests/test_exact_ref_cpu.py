"""Self-checks of tests/exact_ref.py on the CPU: the references the exact GPU tests trust are themselves compared with
something independent (a naive loop nest, float64 autograd), and their magnitudes stay where float32 / bf16 are exact."""
import numpy as np
import torch

from tests import exact_ref as E


def test_generators_are_bf16_exact_and_position_dependent():
    x = E.int_tensor((3, 5, 6, 16))
    assert x.dtype == torch.int64 and int(x.min()) == -3 and int(x.max()) == 3 and E.is_bf16_exact(x)
    # every index moves the value: neighbours along each axis differ somewhere
    for ax in range(4):
        assert bool((x.narrow(ax, 0, x.shape[ax] - 1) != x.narrow(ax, 1, x.shape[ax] - 1)).any())
    d = E.int_tensor((300, 24), coef=(2, 3, 11, 7), mod=5, off=2, salt=2)
    assert int(d.min()) == -2 and int(d.max()) == 2 and E.is_bf16_exact(d)
    w = E.sparse_filter(48, 3, 3, 32)
    assert set(w.unique().tolist()) <= {-1, 0, 1} and int((w != 0).reshape(48, -1).sum(1).max()) <= 5
    assert int((w != 0).sum((0, 3)).min()) > 0                                     # every tap is used by some channel
    wd = E.sparse_filter_dgrad(48, 3, 3, 32)
    assert set(wd.unique().tolist()) <= {-1, 0, 1} and int((wd != 0).permute(3, 0, 1, 2).reshape(32, -1).sum(1).max()) <= 8
    assert int((wd != 0).sum((0, 3)).min()) > 0
    # bf16_rne: exact values stay, ties go to even, and it agrees with torch on float32-representable inputs
    v = torch.tensor([1.0, 1.00390625, 1.01171875, -3.5, 257.0, 259.0, 0.0, 1e-3, 12345.678], dtype=torch.float64)
    got = E.bf16_rne(v)
    assert got.tolist()[:6] == [1.0, 1.0, 1.015625, -3.5, 256.0, 260.0]
    r = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    assert torch.equal(E.bf16_rne(r.double()), r.to(torch.bfloat16).double())
    assert E.is_bf16_exact(got)


def _naive(x, w, dy, stride, pads):
    """The seven loops, int64: y, dx, dw, db."""
    x, w, dy = x.numpy(), w.numpy(), dy.numpy()
    N, H, W, Ci = x.shape
    Co, R, S, _ = w.shape
    _, Ho, Wo, _ = dy.shape
    y, dx, dw = np.zeros((N, Ho, Wo, Co), np.int64), np.zeros_like(x), np.zeros_like(w)
    for n in range(N):
        for oh in range(Ho):
            for ow in range(Wo):
                for k in range(Co):
                    for r in range(R):
                        for s in range(S):
                            ih, iw = oh * stride - pads[0] + r, ow * stride - pads[1] + s
                            if not (0 <= ih < H and 0 <= iw < W):
                                continue
                            for c in range(Ci):
                                y[n, oh, ow, k] += x[n, ih, iw, c] * w[k, r, s, c]
                                dx[n, ih, iw, c] += dy[n, oh, ow, k] * w[k, r, s, c]
                                dw[k, r, s, c] += dy[n, oh, ow, k] * x[n, ih, iw, c]
    return y, dx, dw, dy.reshape(-1, Co).sum(0)


def test_conv_references_equal_the_naive_loops():
    for (N, H, W, Ci, Co, R, S, st, pads) in ((2, 5, 6, 3, 4, 3, 3, 1, (1, 1, 1, 1)), (2, 6, 7, 3, 5, 3, 2, 2, (0, 0, 1, 1))):
        Ho, Wo = E.out_hw(H, W, R, S, st, pads)
        x = E.int_tensor((N, H, W, Ci))
        dy = E.int_tensor((N, Ho, Wo, Co), coef=(2, 3, 11, 7), mod=5, off=2, salt=1)
        w = E.sparse_filter(Co, R, S, Ci, per_out=7) + E.sparse_filter_dgrad(Co, R, S, Ci, per_in=5)
        y, dx, dw, db = _naive(x, w, dy, st, pads)
        assert np.array_equal(E.conv_forward_ref(x, w, st, pads).numpy(), y.astype(np.float64))
        assert np.array_equal(E.conv_dgrad_ref(w, dy, (N, H, W, Ci), st, pads).numpy(), dx.astype(np.float64))
        rw, rb = E.conv_wgrad_ref(x, dy, R, S, st, pads)
        assert np.array_equal(rw.numpy(), dw.astype(np.float64)) and np.array_equal(rb.numpy(), db.astype(np.float64))
        assert np.abs(dx).max() > 0 and np.abs(dw).max() > 0


def test_bn_backward_ref_equals_autograd():
    gen = torch.Generator().manual_seed(3)
    M, Cc = 301, 16
    y = (torch.randn(M, Cc, generator=gen, dtype=torch.float64) * 1.5 + 0.3)
    beta = torch.randn(Cc, generator=gen, dtype=torch.float64) * 0.3
    da = torch.randn(M, Cc, generator=gen, dtype=torch.float64)
    for relu in (True, False):
        yr, br = y.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        mean, var = yr.mean(0), yr.var(0, unbiased=False)
        a = (yr - mean) * torch.rsqrt(var + 0.001) + br
        a = torch.relu(a) if relu else a
        a.backward(da)
        m, r = mean.detach(), torch.rsqrt(var.detach() + 0.001)
        for mask in ((E.mask_from_y(y, m, r, beta), E.mask_from_activation(a.detach()), E.mask_from_threshold(y, m - beta / r))
                     if relu else (None,)):
            dy, dbeta = E.bn_backward_ref(da, y, m, r, M, mask, dbeta_in=3.0)
            assert torch.allclose(dbeta - 3.0, br.grad, rtol=1e-12, atol=1e-12)
            assert torch.allclose(dy, yr.grad, rtol=1e-10, atol=1e-11 * float(yr.grad.abs().max()))


def test_reference_magnitudes_are_exact_in_float32():
    rows = E.exact_magnitudes()
    assert len(rows) > 40
    for label, mx, limit in rows:
        assert 0 < mx and (mx <= limit if limit <= E.BF16_INT_LIMIT else mx < limit), (label, mx, limit)
    # ... and no part of a reduction range is left without weight (a filter whose taps all sat in the first K slice of the
    # split-K case let a reduce that skipped the last slice pass)
    for label, cover in E.filter_coverage():
        assert cover > 0, label
