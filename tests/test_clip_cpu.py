"""CLIP_GRADIENT_NORM without a device: the config key, the float64 oracle (tests/clip_oracle.py) against
torch.nn.utils.clip_grad_norm_ and a hand-computed case, and the argument checks of the new entry points (they come before
any launch, so no GPU is needed)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import clip_oracle as CO

INVALID = -1                                                   # MBX_ERR_INVALID_ARG (include/mbx.h)


@pytest.mark.parametrize("value,want", [(0.5, 0.5), (10, 10.0), (float("inf"), float("inf")), (None, None)])
def test_grad_clip_accepts(value, want):
    from multibox_amd.config import Cfg, grad_clip
    got = grad_clip(Cfg({"CLIP_GRADIENT_NORM": value}))
    assert got == want and (got is None or isinstance(got, float))
    assert grad_clip(Cfg({})) is None


def test_grad_clip_reads_yaml_spellings(tmp_path):
    from multibox_amd.config import grad_clip, parse_config_file, with_defaults
    for text, want in (("CLIP_GRADIENT_NORM: .inf\n", float("inf")), ("CLIP_GRADIENT_NORM: 10\n", 10.0),
                       ("CLIP_GRADIENT_NORM: null\n", None), ("BATCH_SIZE: 2\n", None)):
        f = tmp_path / "c.yaml"
        f.write_text(text)
        assert grad_clip(with_defaults(parse_config_file(str(f)))) == want
    f.write_text("CLIP_GRADIENT_NORM: .nan\n")
    with pytest.raises(ValueError, match="CLIP_GRADIENT_NORM"):
        grad_clip(with_defaults(parse_config_file(str(f))))


@pytest.mark.parametrize("value", [0, -1, True, "1", [1], float("nan"), 0.0, -0.5, False])
def test_grad_clip_rejects(value):
    from multibox_amd.config import Cfg, grad_clip
    with pytest.raises(ValueError, match="CLIP_GRADIENT_NORM"):
        grad_clip(Cfg({"CLIP_GRADIENT_NORM": value}))


@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e9, float("inf")])
def test_oracle_agrees_with_torch_clip_grad_norm(max_norm):
    import torch
    rng = np.random.RandomState(0)
    gs = [rng.randn(n) * s for n, s in ((7, 1.0), (1, 3.0), (1000, 0.05))]
    params = [torch.nn.Parameter(torch.zeros(len(g), dtype=torch.float64)) for g in gs]
    for p, g in zip(params, gs):
        p.grad = torch.from_numpy(g.copy())
    total = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, scale, clipped = CO.clip([(g, None, 0.0) for g in gs], max_norm)
    assert math.isclose(norm, total, rel_tol=1e-14)
    assert (scale < 1.0) == (total > max_norm)
    for p, c in zip(params, clipped):
        # torch multiplies by max_norm / (norm + 1e-6): that epsilon is the whole difference
        assert np.allclose(p.grad.numpy(), c, rtol=1e-5, atol=0)
    blk = CO.clip_block([(g, None, 0.0) for g in gs], max_norm)
    assert blk[2] == np.float32(scale) and blk[3] == np.float32(norm) and blk[4] == float(scale < 1.0) and blk[1] == 0


def test_oracle_hand_computed_with_weight_decay():
    # g' = g + wd * w = (3, 0, 4) + 0.5 * (0, 8, 0) = (3, 4, 4): norm = sqrt(41)
    g, w, wd = np.array([3, 0, 4], np.float32), np.array([0, 8, 0], np.float32), 0.5
    assert math.isclose(CO.global_norm([(g, w, wd)]), math.sqrt(41.0), rel_tol=1e-15)
    norm, scale, (c,) = CO.clip([(g, w, wd)], 2.0)
    assert math.isclose(scale, 2.0 / math.sqrt(41.0), rel_tol=1e-15)
    assert np.allclose(c, np.array([3, 4, 4]) * 2.0 / math.sqrt(41.0), rtol=1e-15)
    assert math.isclose(float(np.sqrt((c ** 2).sum())), 2.0, rel_tol=1e-15)
    # two ranges, the second without decay: (3, 4, 4) and (2,) -> sqrt(45); under the bound nothing changes
    norm, scale, cs = CO.clip([(g, w, wd), (np.array([2.0], np.float32), None, 0.0)], 7.0)
    assert math.isclose(norm, math.sqrt(45.0), rel_tol=1e-15) and scale == 1.0
    assert np.array_equal(cs[0], [3, 4, 4]) and np.array_equal(cs[1], [2])
    assert CO.clip_scale(0.0, 1.0) == 1.0
    # a non-finite element: flagged, not clipped, scale 1; an already flagged block is carried
    blk = CO.clip_block([(np.array([1, np.inf], np.float32), None, 0.0)], 1.0, ctl=(0.0, 2.0))
    assert blk[0] == 0 and blk[1] == 3 and blk[2] == 1 and blk[4] == 0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from multibox_amd import _lib
    return _lib.lib()


def test_new_entry_points_reject_bad_arguments(lib):
    """Pointers here are made-up addresses: every call must be refused before anything is launched or read."""
    A, ODD = 0x10000, 0x10004
    assert lib.mbx_grad_sqnorm_partials(0) == 0 and lib.mbx_grad_sqnorm_partials(-5) == 0
    assert lib.mbx_grad_sqnorm_partials(1) == 1 and lib.mbx_grad_sqnorm_partials(1025) == 2
    assert lib.mbx_grad_sqnorm_partials(1 << 40) == lib.mbx_grad_sqnorm_partials(1 << 30)      # the grid is capped
    sq = lib.mbx_grad_sqnorm
    assert sq(None, A, 8, 0.5, A, None) == INVALID            # g
    assert sq(A, None, 8, 0.5, A, None) == INVALID            # w with wd != 0
    assert sq(A, A, 0, 0.5, A, None) == INVALID and sq(A, A, -3, 0.5, A, None) == INVALID
    assert sq(A, A, 8, 0.5, None, None) == INVALID            # partials
    assert sq(A, A, 8, 0.5, ODD, None) == INVALID             # partials not 8-byte aligned
    fin = lib.mbx_clip_finalize
    assert fin(None, 4, 1.0, A, A, A, None) == INVALID
    assert fin(ODD, 4, 1.0, A, A, A, None) == INVALID
    assert fin(A, 0, 1.0, A, A, A, None) == INVALID and fin(A, -1, 1.0, A, A, A, None) == INVALID
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        assert fin(A, 4, bad, A, A, A, None) == INVALID, bad
    assert fin(A, 4, 1.0, None, A, A, None) == INVALID        # ctl
    assert fin(A, 4, 1.0, A, None, A, None) == INVALID        # clip
    assert fin(A, 4, 1.0, A, A, None, None) == INVALID        # counts
    step = lib.mbx_rmsprop_ema_step_clipped
    args = lambda **kw: [kw.get(k, d) for k, d in (("w", A), ("g", A), ("ms", A), ("mom", None), ("ema", A), ("wb", A), ("n", 8),
                                                   ("lr", 0.01), ("decay", 0.9), ("momentum", 0.0), ("eps", 1.0), ("wd", 4e-5),
                                                   ("d", 0.999), ("on", 1), ("reg", None), ("clip", A), ("stream", None))]
    assert step(*args(clip=None)) == INVALID
    assert step(*args(w=None)) == INVALID and step(*args(n=0)) == INVALID
    assert step(*args(g=None)) == INVALID and step(*args(ms=None)) == INVALID
    assert step(*args(momentum=0.9)) == INVALID               # momentum without its slot
