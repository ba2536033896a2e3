"""Launchers of every form of the batch-norm backward for the exact and the float64-anchored tests: host tensors in, host
float64 (dy, dbeta) out.  Each puts the gradient into a wider view whose other channels are NaN (neither read nor written),
starts dbeta at `dbeta_in` (the kernels accumulate) and keeps a guard row behind dy."""
import ctypes as C

PLAIN_PATHS = ["three_launch", "three_launch_act", "three_launch_mapped", "onepass", "onepass_192", "onepass_mapped", "rows"]
GUARD = 7.0


def _S(torch):
    return torch.cuda.current_stream().cuda_stream


def _f32(torch, t):
    return t.to(torch.float32).contiguous().cuda()


def _wide(torch, da, mapped):
    """da [M, C] -> (device buffer, pointer of the view, ld, channel map or None, column of channel c)."""
    from multibox_amd import _lib
    M, Cc = da.shape
    ld = Cc + 32
    col = [8 + c + (16 if mapped and c >= 8 else 0) for c in range(Cc)]
    wide = torch.full((M, ld), float("nan"), dtype=torch.bfloat16)
    wide[:, col] = da.to(torch.bfloat16)
    dev = wide.cuda()
    cm = None
    if mapped:
        cm = _lib.ChanMap()
        cm.n, cm.c_begin[0], cm.offset[0], cm.c_begin[1], cm.offset[1] = 2, 0, 0, 8, 16
    return dev, wide, dev.data_ptr() + 2 * 8, ld, cm


def path_accepts(path, M, Cc, relu, have_act):
    from multibox_amd import _lib
    l = _lib.lib()
    if path.endswith("mapped") and Cc < 16:
        return False
    if path == "three_launch_act":
        return bool(relu) and have_act
    if path.startswith("onepass"):
        return bool(l.mbx_bn_bwd_onepass_supported(M, Cc, 192 if path == "onepass_192" else 0))
    if path == "rows":
        return Cc <= 2048
    return True


def run_plain(torch, path, da, y, mean, rstd, beta, relu, dbeta_in, act=None, thr=None):
    """One of PLAIN_PATHS.  da / y [M, C] (bf16-exact values), mean / rstd / beta / dbeta_in [C]; act: the stored activation
    (three_launch_act); thr: the relu threshold on y (rows; None with relu = 0: everything passes)."""
    from multibox_amd import _lib
    l = _lib.lib()
    M, Cc = da.shape
    mapped = path.endswith("mapped")
    dev, wide, da_ptr, ld, cm = _wide(torch, da, mapped)
    yd = y.to(torch.bfloat16).contiguous().cuda()
    md, rd, bd = _f32(torch, mean), _f32(torch, rstd), _f32(torch, beta)
    dbeta = _f32(torch, dbeta_in).clone()
    dy = torch.full((M + 1, Cc), GUARD, dtype=torch.bfloat16, device="cuda")
    cmr = None if cm is None else C.byref(cm)
    if path.startswith("three_launch"):
        ad, a_ptr, ld_a = None, None, 0
        if path == "three_launch_act":
            ad = torch.zeros((M, Cc + 8), dtype=torch.bfloat16)
            ad[:, 8:] = act.to(torch.bfloat16)
            ad = ad.cuda()
            a_ptr, ld_a = ad.data_ptr() + 16, Cc + 8
        rows = l.mbx_bn_bwd_rows(M, Cc)
        part = torch.full((rows, Cc, 2), float("nan"), device="cuda")
        m12 = torch.zeros(2 * Cc, device="cuda")
        args = (da_ptr, ld, a_ptr, ld_a, int(relu), yd.data_ptr(), M, Cc, md.data_ptr(), rd.data_ptr(), bd.data_ptr())
        if mapped:
            _lib.check(l.mbx_bn_bwd_reduce_mapped(*args, part.data_ptr(), cmr, _S(torch)))
        else:
            _lib.check(l.mbx_bn_bwd_reduce(*args, part.data_ptr(), _S(torch)))
        _lib.check(l.mbx_bn_bwd_finalize(part.data_ptr(), rows, Cc, M, dbeta.data_ptr(), m12.data_ptr(), _S(torch)))
        if mapped:
            _lib.check(l.mbx_bn_bwd_apply_mapped(*args, m12.data_ptr(), dy.data_ptr(), cmr, _S(torch)))
        else:
            _lib.check(l.mbx_bn_bwd_apply(*args, m12.data_ptr(), dy.data_ptr(), _S(torch)))
    elif path.startswith("onepass"):
        max_wg = 192 if path == "onepass_192" else 0
        assert l.mbx_bn_bwd_onepass_supported(M, Cc, max_wg) == 1
        ws = torch.zeros(l.mbx_bn_bwd_onepass_workspace_bytes(Cc) // 4, device="cuda")
        _lib.check(l.mbx_bn_bwd_onepass_mapped(da_ptr, ld, int(relu), yd.data_ptr(), M, Cc, md.data_ptr(), rd.data_ptr(), bd.data_ptr(),
                                               dbeta.data_ptr(), dy.data_ptr(), ws.data_ptr(), max_wg, None, cmr, _S(torch)))
        torch.cuda.synchronize()
        flags = ws[8 * 2 * Cc:8 * 2 * Cc + 2].view(torch.int32).tolist()
        assert flags[1] == 0 and flags[0] > 0, "grid barrier timed out"
    else:
        assert path == "rows"
        t64 = torch.full((Cc,), float("-inf"), dtype=torch.float64) if thr is None else thr.double()
        td = _f32(torch, t64)
        g = torch.where(y.double() > td.cpu().double(), da.double(), torch.zeros((), dtype=torch.float64))
        table = torch.zeros((8, Cc, 2), dtype=torch.float64)
        for r in range(8):                                  # the sums as eight adders would leave them: rows m = r (mod 8)
            table[r, :, 0] = g[r::8].sum(0)
            table[r, :, 1] = (g[r::8] * y.double()[r::8]).sum(0)
        tab = _f32(torch, table)
        _lib.check(l.mbx_bn_bwd_apply_rows(tab.data_ptr(), 8, da_ptr, ld, yd.data_ptr(), M, Cc, md.data_ptr(), rd.data_ptr(),
                                           td.data_ptr(), dbeta.data_ptr(), dy.data_ptr(), cmr, _S(torch)))
    torch.cuda.synchronize()
    assert bool((dy[M] == GUARD).all()), "guard row behind dy written"
    back = dev.cpu()
    same = (back.view(torch.int16) == wide.view(torch.int16))
    assert bool(same.all()), "the gradient view or its neighbours were written"
    return dy[:M].double().cpu(), dbeta.double().cpu()


def pooled_inputs(torch, act, gy_shape):
    """The pool's argmax from mbx_maxpool_fwd on the activation `act` [N, H, W, C] (host, bf16-exact); -> device uint8."""
    from multibox_amd import _lib
    l = _lib.lib()
    N, H, W, Cc = act.shape
    Ho, Wo = gy_shape[1], gy_shape[2]
    ad = act.to(torch.bfloat16).contiguous().cuda()
    p = torch.zeros((N, Ho, Wo, Cc), dtype=torch.bfloat16, device="cuda")
    arg = torch.zeros((N, Ho, Wo, Cc), dtype=torch.uint8, device="cuda")
    _lib.check(l.mbx_maxpool_fwd(ad.data_ptr(), H * W * Cc, Cc, N, H, W, Cc, 3, 2, p.data_ptr(), Ho * Wo * Cc, Cc, Ho, Wo,
                                 arg.data_ptr(), _S(torch)))
    torch.cuda.synchronize()
    return arg


def pooled_reference_da(torch, act, gy):
    """What the 3x3 / 2 max-pool's backward routes to every pixel: float64 autograd through F.max_pool2d (first maximum), and
    the index tensor [N, C, Ho, Wo] of the pixel (h * W + w) every output reads."""
    import torch.nn.functional as F
    ar = act.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    p, idx = F.max_pool2d(ar, 3, 2, return_indices=True)
    p.backward(gy.double().permute(0, 3, 1, 2))
    return ar.grad.permute(0, 2, 3, 1).contiguous(), idx


def run_pooled(torch, gy, arg, shape, y, mean, rstd, beta, relu, dbeta_in):
    from multibox_amd import _lib
    l = _lib.lib()
    N, H, W, Cc = shape
    Ho, Wo = gy.shape[1], gy.shape[2]
    M = N * H * W
    gyd = gy.to(torch.bfloat16).contiguous().cuda()
    yd = y.to(torch.bfloat16).contiguous().cuda()
    md, rd, bd = _f32(torch, mean), _f32(torch, rstd), _f32(torch, beta)
    dbeta = _f32(torch, dbeta_in).clone()
    rows = l.mbx_bn_bwd_rows_pooled(N, H, W, Cc)
    part = torch.full((rows, Cc, 2), float("nan"), device="cuda")
    m12 = torch.zeros(2 * Cc, device="cuda")
    dy = torch.full((M + 1, Cc), GUARD, dtype=torch.bfloat16, device="cuda")
    geo = (gyd.data_ptr(), Ho * Wo * Cc, Cc, arg.data_ptr(), N, H, W, Ho, Wo, int(relu), yd.data_ptr(), Cc, md.data_ptr(), rd.data_ptr(),
           bd.data_ptr())
    _lib.check(l.mbx_bn_bwd_reduce_pooled(*geo, part.data_ptr(), _S(torch)))
    _lib.check(l.mbx_bn_bwd_finalize(part.data_ptr(), rows, Cc, M, dbeta.data_ptr(), m12.data_ptr(), _S(torch)))
    _lib.check(l.mbx_bn_bwd_apply_pooled(*geo, m12.data_ptr(), dy.data_ptr(), _S(torch)))
    torch.cuda.synchronize()
    assert bool((dy[M] == GUARD).all()), "guard row behind dy written"
    return dy[:M].double().cpu(), dbeta.double().cpu()


def run_fused_tail(torch, g, cfg, cap, dyX, wd, rscale, layers):
    """The data gradient of convolution X (forward geometry g, filter wd [Co][R][S][Ci]) with the batch-norm backward of the
    layers its input is made of as the launch's tail (mbx_conv_desc.bn_bwd).  layers: dicts K, y [M, K], mean, rstd, beta, relu,
    dbeta_in.  -> da [M, Ci] float64 as stored, [(dy, dbeta)] per layer."""
    from multibox_amd import ops, _lib
    l = _lib.lib()
    N, H, W, Ci, Co, R, S, st, pads = g
    Ho, Wo = (H + pads[0] + pads[2] - R) // st + 1, (W + pads[1] + pads[3] - S) // st + 1
    M = N * H * W
    dyb = ops.View.alloc(N, Ho, Wo, Co)
    dyb.tensor().copy_(dyX.to(torch.bfloat16))
    wT = wd.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(torch.bfloat16).cuda()
    da = ops.View.alloc(N, H, W, Ci + 16, zero=True).slice(8, Ci)
    d = ops.make_desc(dyb, wT, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], da, transposed=1, rscale=rscale)
    d.tile_config, d.max_workgroups = cfg, cap
    t = ops.BnBwdFused()
    bar = torch.zeros(ops.GRID_BARRIER_BYTES // 4 + 32, dtype=torch.int32, device="cuda")
    boff = (-(bar.data_ptr() // 4)) % 32
    ctl = torch.zeros(8, device="cuda")
    t.barrier, t.n, t.step_poison = bar.data_ptr() + 4 * boff, len(layers), ctl.data_ptr()
    keep, outs, c0 = [], [], 0
    for i, L in enumerate(layers):
        K = L["K"]
        yd = L["y"].to(torch.bfloat16).contiguous().cuda()
        md, rd, bd = _f32(torch, L["mean"]), _f32(torch, L["rstd"]), _f32(torch, L["beta"])
        dbeta = _f32(torch, L["dbeta_in"]).clone()
        dy = torch.full((M + 1, K), GUARD, dtype=torch.bfloat16, device="cuda")
        acc = torch.zeros((ops.BN_BWD_SLOTS, 2, K), device="cuda")
        t.c_begin[i] = c0
        t.y[i], t.ld_y[i], t.dy[i], t.ld_dy[i] = yd.data_ptr(), K, dy.data_ptr(), K
        t.mean[i], t.rstd[i], t.beta[i], t.dbeta[i] = md.data_ptr(), rd.data_ptr(), bd.data_ptr(), dbeta.data_ptr()
        t.acc[i], t.acc_ld[i], t.relu[i] = acc.data_ptr(), K, int(L["relu"])
        keep.append((yd, md, rd, bd, acc))
        outs.append((dy, dbeta))
        c0 += K
    d.bn_bwd = C.addressof(t)
    assert l.mbx_conv_supported(C.byref(d)) == 0
    ops.conv(d)
    torch.cuda.synchronize()
    assert int(bar[boff + 1]) == 0 and float(ctl[0]) == 0.0 and int(bar[boff]) > 0, "grid barrier timed out / tail did not run"
    full = da.buf.reshape(M, Ci + 16)
    assert float(full[:, :8].float().abs().max()) == 0 and float(full[:, 8 + Ci:].float().abs().max()) == 0
    for dy, _ in outs:
        assert bool((dy[M] == GUARD).all()), "guard row behind dy written"
    return da.tensor().reshape(M, Ci).double().cpu(), [(dy[:M].double().cpu(), db.double().cpu()) for dy, db in outs]
