"""Order-independent, bit-exact checks of every training-path kernel that sums over pixels: weight / bias gradient (single
layer and grouped), the convolution's batch-norm statistics, the bn_bwd_stats epilogue and the five forms of the batch-norm
backward.

Principle (tests/exact_ref.py): with small-integer bf16 inputs every MFMA product and every float32 partial sum is an integer
below 2^24, so the result is the same bits for any tiling, pixel split, atomic arrival order or workgroup count -- and one
pixel dropped, counted twice or read from the wrong address changes it.  Every assertion on a sum is torch.equal against the
int64 / float64 reference; each test first asserts that the reference stays below 2^24 (bf16 outputs: <= 256).

The launches are those of tests/test_gpu_conv.py and tests/test_gpu_nnops.py (same geometries and tile configurations): only
the data is new.
"""
import ctypes as C

import pytest

from tests import bn_bwd_paths as P
from tests import exact_ref as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()
    return torch


def _exact(t, limit=E.EXACT_LIMIT):
    assert 0 < int(t.abs().max()) and (int(t.abs().max()) <= limit if limit <= E.BF16_INT_LIMIT else int(t.abs().max()) < limit)


def _upload(torch, ops, t, pad, off):
    """Host integer tensor [N,H,W,C] -> a channel slice of a wider zeroed bf16 buffer."""
    N, H, W, Cc = t.shape
    v = ops.View.alloc(N, H, W, Cc + pad, zero=True).slice(off, Cc)
    v.tensor().copy_(t.to(torch.bfloat16))
    return v


def _outside_zero(torch, v):
    full = v.buf.reshape(v.N, v.H, v.W, v.ld).float()
    return float(full[..., :v.ch_off].abs().max() if v.ch_off else 0.0) == 0 and \
        float(full[..., v.ch_off + v.C:].abs().max() if v.ch_off + v.C < v.ld else 0.0) == 0


# ------------------------------------------------------------------------------------------------ (a) single-layer launches
@pytest.mark.parametrize("name", E.SINGLE_WGRAD)
def test_single_layer_wgrad_forward_dgrad_exact(T, name):
    """mbx_conv_wgrad at tile_config 0..11 and mbx_conv_wgrad_scaled (0.25): dw / db equal the integer reference, and a second
    launch without clearing leaves exactly twice it (the launches accumulate); forward and data gradient at tile_config 0 equal
    theirs.  Includes M = 36 (less than one 64-pixel step), stride 2 with asymmetric padding, and the 25-channel head whose dy
    is padded to ld 32."""
    torch = T
    from multibox_amd import ops, _lib
    l = _lib.lib()
    c = E.conv_case(name)
    N, H, W, Ci, Co, R, S, st, pads = c["g"]
    Ho, Wo = c["Ho"], c["Wo"]
    _exact(2 * c["dw"]), _exact(2 * c["db"])
    xb = _upload(torch, ops, c["x"], 8, 8)
    head = name == "head_25"
    if head:
        dyb = ops.View.alloc(N, Ho, Wo, Co, ld=32, zero=True)
        dyb.tensor().copy_(c["dy"].to(torch.bfloat16))
    else:
        dyb = _upload(torch, ops, c["dy"], 8, 8)
    dw = torch.zeros((Co, R, S, Ci), dtype=torch.float32, device="cuda")
    db = torch.zeros((32 if head else Co,), dtype=torch.float32, device="cuda")
    d = ops.make_desc(xb, None, Co, R, S, st, pads[0], pads[1], ops.View.alloc(N, Ho, Wo, 32 if head else Co))
    d.C_out = Co
    ref_w, ref_b = c["dw"].float(), c["db"].float()
    for cfg in range(12):
        d.tile_config = cfg
        dw.zero_(); db.zero_()
        for rep in (1, 2):
            ops.conv_wgrad(d, dyb, dw, db)
            torch.cuda.synchronize()
            assert torch.equal(dw.cpu(), rep * ref_w), "dw tile_config %d launch %d: %d elements differ" % (
                cfg, rep, int((dw.cpu() != rep * ref_w).sum()))
            assert torch.equal(db[:Co].cpu(), rep * ref_b), "db tile_config %d launch %d" % (cfg, rep)
            assert float(db[Co:].abs().sum()) == 0
    d.tile_config = 0
    dw.zero_(); db.zero_()
    _lib.check(l.mbx_conv_wgrad_scaled(C.byref(d), dyb.ptr, dyb.img_stride, dyb.ld, 0.25, dw.data_ptr(), db.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), 0.25 * ref_w) and torch.equal(db[:Co].cpu(), 0.25 * ref_b)
    if head:
        return
    # forward and data gradient (sparse integer filters: outputs exact in bf16), slices of wider buffers
    _exact(c["y"], E.BF16_INT_LIMIT), _exact(c["dx"], E.BF16_INT_LIMIT)
    yb = ops.View.alloc(N, Ho, Wo, Co + 24, zero=True).slice(16, Co)
    wdev = c["w"].to(torch.bfloat16).cuda().contiguous()
    ops.conv(ops.make_desc(xb, wdev, Co, R, S, st, pads[0], pads[1], yb))
    torch.cuda.synchronize()
    assert torch.equal(yb.tensor().float().cpu(), c["y"].float()), "forward"
    assert _outside_zero(torch, yb)
    wT = c["wd"].flip(1, 2).permute(3, 1, 2, 0).contiguous().to(torch.bfloat16).cuda()       # [Ci][R][S][Co]
    dx = ops.View.alloc(N, H, W, Ci + 8, zero=True).slice(0, Ci)
    ops.conv(ops.make_desc(dyb, wT, Ci, R, S, st, R - 1 - pads[0], S - 1 - pads[1], dx, transposed=1))
    torch.cuda.synchronize()
    assert torch.equal(dx.tensor().float().cpu(), c["dx"].float()), "data gradient"
    assert _outside_zero(torch, dx)


# M = 36 (less than one 64-pixel step), the linear 1x1 path, general addressing with C_out below one narrow tile's width
WGRAD_EDGE_CASES = ["2x2_valid_128_96", "1x1_320_96", "3x3_same_32_48"]


@pytest.mark.parametrize("name", WGRAD_EDGE_CASES)
def test_single_layer_wgrad_no_bias_exact(T, name):
    """mbx_conv_wgrad with db = NULL (the instantiations without the bias gradient, which the test above never launches) at
    tile_config 0..11: dw equals the integer reference after one launch and exactly twice it after two."""
    torch = T
    from multibox_amd import ops
    c = E.conv_case(name)
    N, H, W, Ci, Co, R, S, st, pads = c["g"]
    Ho, Wo = c["Ho"], c["Wo"]
    _exact(2 * c["dw"])
    xb = _upload(torch, ops, c["x"], 8, 8)
    dyb = _upload(torch, ops, c["dy"], 8, 8)
    dw = torch.zeros((Co, R, S, Ci), dtype=torch.float32, device="cuda")
    d = ops.make_desc(xb, None, Co, R, S, st, pads[0], pads[1], ops.View.alloc(N, Ho, Wo, Co))
    ref_w = c["dw"].float()
    for cfg in range(12):
        d.tile_config = cfg
        dw.zero_()
        for rep in (1, 2):
            ops.conv_wgrad(d, dyb, dw, None)
            torch.cuda.synchronize()
            assert torch.equal(dw.cpu(), rep * ref_w), "dw tile_config %d launch %d: %d elements differ" % (
                cfg, rep, int((dw.cpu() != rep * ref_w).sum()))


@pytest.mark.parametrize("name", WGRAD_EDGE_CASES)
def test_single_layer_wgrad_nondense_dy_exact(T, name):
    """mbx_conv_wgrad_scaled on a dy with a gap of three pixel rows between images (dy_img_stride = (H_out W_out + 3) ld_dy,
    the gap filled with a non-zero value), at tile_config 0, 2, 7 and 9 -- at 7 and 9 the library must fall back to the wide
    tile, the narrow one needs dense dy: dw and db equal the integer reference, i.e. no gap row is ever summed."""
    torch = T
    from multibox_amd import ops, _lib
    l = _lib.lib()
    c = E.conv_case(name)
    N, H, W, Ci, Co, R, S, st, pads = c["g"]
    Ho, Wo = c["Ho"], c["Wo"]
    _exact(c["dw"]), _exact(c["db"])
    assert Co % 8 == 0
    xb = _upload(torch, ops, c["x"], 8, 8)
    ld, rows = Co, Ho * Wo + 3
    dyg = torch.full((N, rows, ld), 3.0, dtype=torch.bfloat16, device="cuda")
    dyg[:, :Ho * Wo, :] = c["dy"].reshape(N, Ho * Wo, Co).to(torch.bfloat16).cuda()
    dw = torch.zeros((Co, R, S, Ci), dtype=torch.float32, device="cuda")
    db = torch.zeros((Co,), dtype=torch.float32, device="cuda")
    d = ops.make_desc(xb, None, Co, R, S, st, pads[0], pads[1], ops.View.alloc(N, Ho, Wo, Co))
    ref_w, ref_b = c["dw"].float(), c["db"].float()
    for cfg in (0, 2, 7, 9):
        d.tile_config = cfg
        dw.zero_(); db.zero_()
        _lib.check(l.mbx_conv_wgrad_scaled(C.byref(d), dyg.data_ptr(), rows * ld, ld, 1.0, dw.data_ptr(), db.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(dw.cpu(), ref_w), "dw tile_config %d: %d elements differ" % (cfg, int((dw.cpu() != ref_w).sum()))
        assert torch.equal(db.cpu(), ref_b), "db tile_config %d" % cfg


# ------------------------------------------------------------------------------------------------ (b) grouped weight gradient
@pytest.mark.parametrize("flags", [0, 1, 2], ids=["default", "deterministic", "scatter"])
@pytest.mark.parametrize("plan", ["A", "B"])
def test_grouped_wgrad_exact(T, monkeypatch, plan, flags):
    """mbx_conv_wgrad_grouped on integer data: plan A = the job list of test_wgrad_grouped_matches_reference_and_single_layer_api,
    plan B = one 8 x 35 x 35 3x3 layer alone (which the default plan must split: the plain-store and the atomic paths see the
    same data).  Default / deterministic / scatter plans; the same device image launched uncapped, with 24 workgroups, and
    uncapped again (dw / db cleared in between; the kernel resets the queue heads): every result equals the reference."""
    torch = T
    from multibox_amd import ops
    if flags & 2:
        monkeypatch.setenv("MBX_WGRAD_SCATTER", "1")
    else:
        monkeypatch.delenv("MBX_WGRAD_SCATTER", raising=False)
    names = E.GROUP_PLAN_A if plan == "A" else E.GROUP_PLAN_B
    jobs, checks, keep = [], [], []
    for i, name in enumerate(names):
        c = E.conv_case(name)
        N, H, W, Ci, Co, R, S, st, pads = c["g"]
        Ho, Wo = c["Ho"], c["Wo"]
        scale = 0.5 if i % 3 == 0 else 1.0
        use_bias = (i % 3 == 0)
        _exact(c["dw"]), _exact(c["db"])
        xb = _upload(torch, ops, c["x"], 8, 8) if i % 2 else _upload(torch, ops, c["x"], 0, 0)
        ld = (Co + 7) // 8 * 8
        dyb = ops.View.alloc(N, Ho, Wo, Co, ld=ld, zero=True)
        dyb.tensor().copy_(c["dy"].to(torch.bfloat16))
        dw = torch.zeros((Co, R, S, Ci), dtype=torch.float32, device="cuda")
        db = torch.zeros((Co,), dtype=torch.float32, device="cuda") if use_bias else None
        j = ops.WgradJob()
        j.desc = ops.make_desc(xb, None, Co, R, S, st, pads[0], pads[1], ops.View(dyb.buf, N, Ho, Wo, 8, ld, 0, 2))
        j.desc.C_out = Co
        j.dy, j.dy_img_stride, j.ld_dy, j.scale = dyb.ptr, dyb.img_stride, dyb.ld, scale
        j.dw, j.db = dw.data_ptr(), (None if db is None else db.data_ptr())
        jobs.append(j)
        keep.append((xb, dyb))
        checks.append((name, dw, db, c["dw"].float() * scale, c["db"].float() * scale))
    grp = ops.WgradGroup(jobs, deterministic=bool(flags & 1))
    assert grp.info.n_layers == len(jobs) and grp.info.n_items >= len(jobs)
    if plan == "B":
        det = ops.WgradGroup(jobs, deterministic=True)
        if flags & 1:
            assert grp.info.n_items == det.info.n_items
        else:
            assert grp.info.n_items > det.info.n_items, "the lone layer is not split: the atomic path is not exercised"
    for launch, cap in enumerate((0, 24, 0)):
        for _, dw, db, _, _ in checks:
            dw.zero_()
            if db is not None:
                db.zero_()
        grp.launch(max_workgroups=cap)
        torch.cuda.synchronize()
        for name, dw, db, ref_w, ref_b in checks:
            assert torch.equal(dw.cpu(), ref_w), "%s dw, launch %d (cap %d): %d elements differ" % (
                name, launch, cap, int((dw.cpu() != ref_w).sum()))
            assert db is None or torch.equal(db.cpu(), ref_b), "%s db, launch %d (cap %d)" % (name, launch, cap)
    assert grp.completed_ok()


# ------------------------------------------------------------------------------------------------ (c) convolution statistics
@pytest.mark.parametrize("name", list(E.STATS_CASES))
def test_conv_statistics_exact(T, name):
    """Forward with stats_partial, float rows and 16 fixed-point rows: y equals the integer reference (split-K included), the
    float rows sum to exactly sum y / sum y^2, the fixed-point rows to exactly those times 2^20."""
    torch = T
    from multibox_amd import ops, _lib
    l = _lib.lib()
    c = E.forward_case(name, "stats")
    cfg = E.STATS_CASES[name][1]
    N, H, W, Ci, Co, R, S, st, pads = c["g"]
    Ho, Wo = E.out_hw(H, W, R, S, st, pads)
    y_ref = c["y"]
    flat = y_ref.reshape(-1, Co)
    sums = torch.stack([flat.sum(0), (flat * flat).sum(0)], 1)                   # int64 [Co, 2]
    _exact(y_ref, E.BF16_INT_LIMIT), _exact(sums)
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(c["x"].to(torch.bfloat16))
    wd = c["w"].to(torch.bfloat16).cuda().contiguous()
    keep = []

    def run(stats, mod, ld):
        yb = ops.View.alloc(N, Ho, Wo, Co, zero=True)
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, stats=stats, stats_rows_mod=mod, stats_ld=ld)
        d.tile_config = cfg
        if cfg > 128:
            ws = torch.empty(int(l.mbx_conv_splitk_workspace_bytes(C.byref(d))) // 4, dtype=torch.float32, device="cuda")
            d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
            keep.append(ws)
        assert l.mbx_conv_supported(C.byref(d)) == 0
        ops.conv(d)
        torch.cuda.synchronize()
        return yb

    d0 = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], ops.View.alloc(N, Ho, Wo, Co))
    d0.tile_config = cfg
    rows = ops.conv_stats_rows(d0)
    plain = torch.zeros((rows, Co, 2), dtype=torch.float32, device="cuda")
    y0 = run(plain, 0, 0)
    assert torch.equal(y0.tensor().float().cpu(), y_ref.float()), "y (float rows)"
    assert torch.equal(plain.double().sum(0).cpu(), sums.double()), "float rows"
    table = torch.zeros((16, Co, 2), dtype=torch.int64, device="cuda")
    y1 = run(table, 16, Co)
    assert torch.equal(y1.tensor().float().cpu(), y_ref.float()), "y (fixed-point rows)"
    assert torch.equal(table.sum(0).cpu(), sums * 2 ** 20), "fixed-point rows"


# ------------------------------------------------------------------------------------------------ (d) bn_bwd_stats epilogue
@pytest.mark.parametrize("cfg", [0, 10, 33, "pair"])
def test_bn_bwd_stats_epilogue_exact(T, cfg):
    """The data gradient's {sum g, sum g y} tables (geometry and table layout of test_conv_bn_bwd_stats_epilogue): integer y,
    half-integer thresholds (no element on the mask), gradient = 0.5 x an integer -- the eight rows sum to exactly the
    reference, twice it for the pair launch (both problems add into the same tables)."""
    torch = T
    from multibox_amd import ops, _lib
    l = _lib.lib()
    c = E.forward_case("bw", "bwd_stats")
    N, H, W, Ci, Co, R, S, st, pads = c["g"]
    Ho, Wo = E.out_hw(H, W, R, S, st, pads)
    M = N * Ho * Wo
    stream = torch.cuda.current_stream().cuda_stream
    g_ref = c["y"].double().reshape(M, Co) * 0.5                       # what the launch stores: rscale 0.5, exact in bf16
    xb = ops.View.alloc(N, H, W, Ci)
    xb.tensor().copy_(c["x"].to(torch.bfloat16))
    wd = c["w"].to(torch.bfloat16).cuda().contiguous()
    Y0h, Y1h = E.int_tensor((M, 96)), E.int_tensor((M, 32), salt=3)
    thr0h = (torch.arange(96) % 5 - 2).double() + 0.5
    thr1h = (torch.arange(32) % 3 - 1).double() - 0.5
    thr1h[:8] = float("-inf")                                          # (a layer without relu: everything passes)
    Y0, Y1 = Y0h.to(torch.bfloat16).cuda(), Y1h.to(torch.bfloat16).cuda()
    thr0, thr1 = thr0h.float().cuda(), thr1h.float().cuda()
    st0 = torch.zeros((8, 96, 2), dtype=torch.float32, device="cuda")
    st1 = torch.zeros((8, 48, 2), dtype=torch.float32, device="cuda")
    tab = _lib.BnBwdStats()
    tab.n, tab.rows_mod = 2, 8
    tab.c_begin[0], tab.c_begin[1] = 0, 64
    tab.y[0], tab.ld_y[0], tab.relu_thr[0], tab.stats[0], tab.stats_ld[0] = Y0.data_ptr() + 2 * 16, 96, thr0.data_ptr() + 4 * 16, st0.data_ptr() + 8 * 16, 96
    tab.y[1], tab.ld_y[1], tab.relu_thr[1], tab.stats[1], tab.stats_ld[1] = Y1.data_ptr(), 32, thr1.data_ptr(), st1.data_ptr() + 8 * 8, 48

    def desc(yb):
        d = ops.make_desc(xb, wd, Co, R, S, st, pads[0], pads[1], yb, rscale=0.5)
        d.tile_config = 10 if cfg == "pair" else cfg
        d.bn_bwd_stats = C.addressof(tab)
        return d

    yb = ops.View.alloc(N, Ho, Wo, Co, zero=True)
    if cfg == "pair":
        yc = ops.View.alloc(N, Ho, Wo, Co, zero=True)
        d1, d2 = desc(yb), desc(yc)
        assert l.mbx_conv_pair(C.byref(d1), C.byref(d2), stream) == 0
        scale = 2.0
    else:
        assert l.mbx_conv_supported(C.byref(desc(yb))) == 0
        ops.conv(desc(yb))
        scale = 1.0
    torch.cuda.synchronize()
    assert torch.equal(yb.tensor().reshape(M, Co).double().cpu(), g_ref)
    for (Yh, thr, tb, c_lo, c_n, y_lo, s_lo) in ((Y0h, thr0h, st0, 0, 64, 16, 16), (Y1h, thr1h, st1, 64, 32, 0, 8)):
        yy = Yh[:, y_lo:y_lo + c_n].double()
        assert not bool((yy == thr[y_lo:y_lo + c_n]).any())
        gg = torch.where(yy > thr[y_lo:y_lo + c_n], g_ref[:, c_lo:c_lo + c_n], torch.zeros((), dtype=torch.float64))
        want = torch.stack([gg.sum(0), (gg * yy).sum(0)], 1) * scale
        assert float((gg * yy).abs().sum(0).max()) * scale * 2 < E.EXACT_LIMIT and float(want.abs().max()) > 0
        got = tb[:, s_lo:s_lo + c_n].double().sum(0).cpu()
        assert torch.equal(got, want), (c_lo, int((got != want).sum()), float((got - want).abs().max()))
        assert float(tb[:, :s_lo].abs().max()) == 0 and float(tb[:, s_lo + c_n:].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ (e) batch-norm backward, exact tier
def _exact_masks(torch, e, relu):
    """act (the constructed activation), thr and the mask of the exact tier -- the three mask forms coincide (exact arithmetic)."""
    xh = (e["y"].double() - e["mean"]) * e["rstd"]
    act = torch.relu(xh + e["beta"])
    assert E.is_bf16_exact(act)
    m = E.mask_from_y(e["y"], e["mean"], e["rstd"], e["beta"])
    assert torch.equal(m, E.mask_from_activation(act)) and torch.equal(m, E.mask_from_threshold(e["y"], e["thr"]))
    return act, (m if relu else None)


@pytest.mark.parametrize("path,relu", [("three_launch_act", 1), ("three_launch", 1), ("three_launch", 0), ("three_launch_mapped", 1),
                                       ("three_launch_mapped", 0), ("onepass", 1), ("onepass", 0), ("onepass_192", 1),
                                       ("onepass_mapped", 1), ("rows", 1), ("rows", 0)])
def test_bn_backward_exact(T, path, relu):
    """M = 256, C = 64, integer da / y / mean, rstd = 0.5, half-integer beta: every float32 operation is exact, so dy must be
    the bf16 rounding of the float64 reference bit for bit and dbeta exactly dbeta_in + sum g (dbeta_in = 3)."""
    torch = T
    e = E.bn_exact_case()
    M, Cc = e["y"].shape
    act, mask = _exact_masks(torch, e, relu)
    dbeta_in = torch.full((Cc,), 3.0, dtype=torch.float64)
    dy_ref, dbeta_ref = E.bn_backward_ref(e["da"], e["y"], e["mean"], e["rstd"], M, mask, dbeta_in)
    _exact(dbeta_ref)
    assert P.path_accepts(path, M, Cc, relu, True)
    dy, dbeta = P.run_plain(torch, path, e["da"], e["y"], e["mean"], e["rstd"], e["beta"], relu, dbeta_in, act=act,
                            thr=(e["thr"] if relu else None))
    assert torch.equal(dbeta, dbeta_ref), "dbeta: %d channels differ" % int((dbeta != dbeta_ref).sum())
    want = E.bf16_rne(dy_ref)
    assert torch.equal(dy, want), "dy: %d elements differ, max %.3g" % (int((dy != want).sum()), float((dy - want).abs().max()))
    assert float(dy.abs().max()) > 0


def f64_close(dy, ref):
    """The rule of tests/test_gpu_bn_backward_f64.py: |dy - ref| <= 2^-8 |ref| + 1e-5 max|ref| per channel."""
    err = (dy - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-5 * ref.abs().max(0).values
    bad = err > bound
    return int(bad.sum()) == 0, "%d/%d out of tolerance, max err %.3g, max|ref| %.3g" % (
        int(bad.sum()), bad.numel(), float(err.max()), float(ref.abs().max()))


@pytest.mark.parametrize("relu", [1, 0])
def test_bn_backward_pooled_exact(T, relu):
    """The pooled pair on N = 4, 17 x 17 -> 8 x 8 with an integer pool gradient and the argmax of mbx_maxpool_fwd on the
    constructed activation: the gathered gradient is an integer sum of at most 4 terms.  dbeta is exact; M = 1156 is not a
    power of two, so dy is held to the float64 rule (2^-8 |ref| + 1e-5 max|ref|)."""
    torch = T
    N, H, W, Cc = 4, 17, 17, 64
    M = N * H * W
    e = E.bn_exact_case(M, Cc)
    xh = (e["y"].double() - e["mean"]) * e["rstd"]
    pre = xh + e["beta"]
    act = (torch.relu(pre) if relu else pre).reshape(N, H, W, Cc)
    assert E.is_bf16_exact(act)
    gy = E.int_tensor((N, 8, 8, Cc), coef=(2, 3, 11, 7), mod=5, off=2, salt=4)
    da_ref, _ = P.pooled_reference_da(torch, act, gy)
    da_ref = da_ref.reshape(M, Cc)
    assert float(da_ref.abs().max()) <= 8 and float(da_ref.abs().max()) > 2         # windows overlap: sums of several terms
    mask = E.mask_from_y(e["y"], e["mean"], e["rstd"], e["beta"]) if relu else None
    dbeta_in = torch.full((Cc,), 3.0, dtype=torch.float64)
    dy_ref, dbeta_ref = E.bn_backward_ref(da_ref, e["y"], e["mean"], e["rstd"], M, mask, dbeta_in)
    _exact(dbeta_ref)
    arg = P.pooled_inputs(torch, act, gy.shape)
    dy, dbeta = P.run_pooled(torch, gy, arg, (N, H, W, Cc), e["y"], e["mean"], e["rstd"], e["beta"], relu, dbeta_in)
    assert torch.equal(dbeta, dbeta_ref), "dbeta: %d channels differ" % int((dbeta != dbeta_ref).sum())
    ok, msg = f64_close(dy, dy_ref)
    assert ok, msg


def test_bn_backward_fused_tail_exact(T):
    """The fused tail (mbx_conv_desc.bn_bwd) on b8up (N = 64, 8 x 8: M = 4096, tile_config 33): integer upstream gradient, sparse
    integer filter, rscale = 0 -- da is an integer with |da| <= 16 and equals the data-gradient reference; dy is the bf16
    rounding of the float64 reference bit for bit, dbeta exact, for both layers (with and without relu)."""
    torch = T
    f = E.fused_exact_case()
    N, H, W, Ci, Co, R, S, st, pads = f["g"]
    M = N * H * W
    assert int(f["da"].abs().max()) <= 16
    layers, c0 = [], 0
    for i, K in enumerate(f["split"]):
        e = E.bn_exact_case(M, K)
        layers.append(dict(K=K, y=e["y"] if i == 0 else -e["y"], mean=e["mean"], rstd=e["rstd"], beta=e["beta"], relu=int(i % 2 == 0),
                           dbeta_in=torch.full((K,), 3.0, dtype=torch.float64)))
    da, outs = P.run_fused_tail(torch, f["g"], f["cfg"], f["cap"], f["dyX"], f["wd"], 0.0, layers)
    da_ref = f["da"].double().reshape(M, Ci)
    assert torch.equal(da, da_ref), "da: %d elements differ" % int((da != da_ref).sum())
    for i, (L, (dy, dbeta)) in enumerate(zip(layers, outs)):
        K = L["K"]
        mask = E.mask_from_y(L["y"], L["mean"], L["rstd"], L["beta"]) if L["relu"] else None
        dy_ref, dbeta_ref = E.bn_backward_ref(da_ref[:, c0:c0 + K], L["y"], L["mean"], L["rstd"], M, mask, L["dbeta_in"])
        _exact(dbeta_ref)
        assert torch.equal(dbeta, dbeta_ref), "layer %d dbeta: %d channels differ" % (i, int((dbeta != dbeta_ref).sum()))
        want = E.bf16_rne(dy_ref)
        assert torch.equal(dy, want), "layer %d dy: %d elements differ, max %.3g" % (i, int((dy != want).sum()), float((dy - want).abs().max()))
        c0 += K


# ------------------------------------------------------------------------------------------------ (f) row coverage at ragged M
@pytest.mark.parametrize("M,Cc", E.BN_ROW_SHAPES)
def test_bn_backward_row_coverage(T, M, Cc):
    """da = 1 everywhere, no relu: dbeta must be exactly dbeta_in + M -- every row counted once, whatever the row split.  Then
    da = 2 in rows 0 and M - 1 only: dbeta = dbeta_in + 4 exactly and dy within the float64 rule.  Every plain path that
    accepts the shape."""
    torch = T
    e = E.bn_exact_case(M, Cc)
    dbeta_in = torch.full((Cc,), 3.0, dtype=torch.float64)
    ones = torch.ones((M, Cc), dtype=torch.float64)
    ends = torch.zeros((M, Cc), dtype=torch.float64)
    ends[0], ends[M - 1] = 2.0, 2.0
    ref_ends = E.bn_backward_ref(ends, e["y"], e["mean"], e["rstd"], M, None, dbeta_in)
    ran = 0
    for path in P.PLAIN_PATHS:
        if not P.path_accepts(path, M, Cc, 0, False):
            continue
        _, dbeta = P.run_plain(torch, path, ones, e["y"], e["mean"], e["rstd"], e["beta"], 0, dbeta_in)
        assert torch.equal(dbeta, dbeta_in + M), "%s: dbeta - dbeta_in = %s, M = %d" % (path, sorted(set((dbeta - dbeta_in).tolist()))[:4], M)
        dy, dbeta = P.run_plain(torch, path, ends, e["y"], e["mean"], e["rstd"], e["beta"], 0, dbeta_in)
        assert torch.equal(dbeta, dbeta_in + 4.0), "%s: first / last row" % path
        ok, msg = f64_close(dy, ref_ends[0])
        assert ok, "%s: %s" % (path, msg)
        ran += 1
    assert ran >= 3


# ------------------------------------------------------------------------------------------------ pooling: signs, slices, accumulate
@pytest.mark.parametrize("N,H,W,Cc,k,st", [(3, 9, 9, 8, 3, 2), (2, 12, 13, 16, 2, 2)])
@pytest.mark.parametrize("sign", ["negative", "mixed"])
def test_maxpool_negative_and_mixed_inputs(T, N, H, W, Cc, k, st, sign):
    """mbx_maxpool_fwd on inputs that are all negative / of both signs (a maximum that started from 0 would pass the relu-fed
    test_maxpool): the pooled values equal torch's exactly and the argmax byte is the tap r * k + s of torch's first maximum."""
    torch = T
    import torch.nn.functional as F
    from multibox_amd import _lib, ops
    l = _lib.lib()
    x = E.int_tensor((N, H, W, Cc), mod=13, off=5)                       # -5 .. 7: ties inside most windows
    if sign == "negative":
        x = x - 8
        assert int(x.max()) < 0
    else:
        assert int(x.min()) < 0 < int(x.max())
    Ho, Wo = (H - k) // st + 1, (W - k) // st + 1
    yr, idx = F.max_pool2d(x.double().permute(0, 3, 1, 2), k, st, return_indices=True)
    oh = torch.arange(Ho).reshape(1, 1, Ho, 1)
    ow = torch.arange(Wo).reshape(1, 1, 1, Wo)
    tap = (idx // W - oh * st) * k + (idx % W - ow * st)                 # [N, C, Ho, Wo]
    xv = _upload(torch, ops, x, 8, 0)
    yv = ops.View.alloc(N, Ho, Wo, Cc + 8, zero=True).slice(8, Cc)
    am = torch.full((N, Ho, Wo, Cc), 255, dtype=torch.uint8, device="cuda")
    _lib.check(l.mbx_maxpool_fwd(xv.ptr, xv.img_stride, xv.ld, N, H, W, Cc, k, st, yv.ptr, yv.img_stride, yv.ld, Ho, Wo, am.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(yv.tensor().double().cpu(), yr.permute(0, 2, 3, 1))
    assert torch.equal(am.cpu().long(), tap.permute(0, 2, 3, 1)), "argmax is not the first maximum"
    assert _outside_zero(torch, yv)


def test_avgpool_slices_and_accumulate(T):
    """mbx_avgpool_fwd / _bwd (2 x 35 x 35 x 192, k 3, pad 1) on channel slices of wider buffers, the backward also with
    accumulate = 1 onto an existing gradient: integer data, within one bf16 ulp of the float64 reference (the divisions by
    9 / 6 / 4 valid taps are not exact), neighbours of the slices untouched."""
    torch = T
    import torch.nn.functional as F
    from multibox_amd import _lib, ops
    l = _lib.lib()
    N, H, W, Cc, k, pad = 2, 35, 35, 192, 3, 1
    S = torch.cuda.current_stream().cuda_stream
    x = E.int_tensor((N, H, W, Cc))
    dy = E.int_tensor((N, H, W, Cc), coef=(2, 3, 11, 7), mod=5, off=2, salt=1)
    old = E.int_tensor((N, H, W, Cc), coef=(2, 3, 11, 7), mod=5, off=2, salt=3)
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    yr = F.avg_pool2d(xr, k, 1, pad, count_include_pad=False)
    yr.backward(dy.double().permute(0, 3, 1, 2))
    y_ref, dx_ref = yr.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1)

    def one_ulp(out, ref):
        err = (out.double().cpu() - ref).abs()
        bad = err > ref.abs() * 2.0 ** -7 + 1e-6 * float(ref.abs().max())
        return int(bad.sum()) == 0, "%d/%d beyond one bf16 ulp, max err %.3g" % (int(bad.sum()), bad.numel(), float(err.max()))

    xv = _upload(torch, ops, x, 16, 8)
    yv = ops.View.alloc(N, H, W, Cc + 24, zero=True).slice(16, Cc)
    _lib.check(l.mbx_avgpool_fwd(xv.ptr, xv.img_stride, xv.ld, N, H, W, Cc, k, pad, yv.ptr, yv.img_stride, yv.ld, H, W, S))
    torch.cuda.synchronize()
    ok, msg = one_ulp(yv.tensor(), y_ref)
    assert ok, "forward: " + msg
    assert _outside_zero(torch, yv)
    dyv = _upload(torch, ops, dy, 8, 8)
    for accumulate in (0, 1):
        dxv = _upload(torch, ops, old, 16, 8)
        _lib.check(l.mbx_avgpool_bwd(dyv.ptr, dyv.img_stride, dyv.ld, N, H, W, Cc, k, pad, H, W, dxv.ptr, dxv.img_stride, dxv.ld,
                                     accumulate, S))
        torch.cuda.synchronize()
        ok, msg = one_ulp(dxv.tensor(), dx_ref + (old.double() if accumulate else 0.0))
        assert ok, "backward accumulate %d: %s" % (accumulate, msg)
        assert _outside_zero(torch, dxv)
