"""-m gpu: the fused renderer's ordered work lists (csrc/render_worklist.hpp, render_rays_kernel.hpp) -- exact mode against the CPU oracle, bit for bit,
at the launch shapes where the hand-out takes another path: a grid that is no multiple of 8 (9 rays), more than one chunk per XCD (520), a staggered
start with more items than waves on an XCD, so that tickets are really taken ahead and hand-offs really cross waves (2056); 8 tiles (64+64) and
4 tiles (32+32: fewer than the longest list's items per ray); the pair interleave with per-sample outputs; a field with view directions (the bias rides
in the hand-off state); two launches of different shapes back to back on one stream (the cached lists, the generation tags).  No hand-off ever times out."""
import numpy as np
import pytest
import torch

from tests.common import load_golden, make_rays
from tests.gpu_common import device_field, oracle_field, assert_bitwise
from tests.test_gpu_render import FLOAT_KEYS, _run_both, _compare_bitwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RAY0 = 1024            # first ray taken from the 64 x 64 view: rows 16 .. of 64, body and background


@pytest.fixture(scope="module")
def env(oracle):
    assert torch.cuda.is_available(), "these tests need a GPU"
    p = load_golden("nsr_params.npz")
    f, table = device_field(p)
    ro, rd = make_rays(64, 64, dist=1.7, f=50.0)
    return dict(p=p, f=f, of=oracle_field(p, table), O=oracle, ro=ro, rd=rd, cache={})


def _both(env, n, T0, up):
    """(GPU, oracle) results of rays [RAY0, RAY0 + n), rendered once per shape and shared by the tests (nothing modifies them)"""
    key = (n, T0, up)
    if key not in env["cache"]:
        from avatarcraft_amd import nsr_ops
        g, r = _run_both(env, env["ro"][RAY0:RAY0 + n], env["rd"][RAY0:RAY0 + n], T0, up)
        assert nsr_ops.handoff_timeouts(DEV) == 0
        env["cache"][key] = (g, r)
    return env["cache"][key]


@pytest.mark.parametrize("n", [9, 520, 2056])
def test_eight_tiles_equal_the_oracle(env, n):
    g, r = _both(env, n, 64, 64)
    _compare_bitwise(g, r, 64)
    assert r["weights_sum"].max() > 0.5 or n < 16                     # (the rays do meet the body)


def test_four_tiles_equal_the_oracle(env):
    g, r = _both(env, 520, 32, 32)
    _compare_bitwise(g, r, 32)


def test_pair_launch_with_per_sample_outputs(env):
    from avatarcraft_amd import nsr_ops
    n = 520
    ro, rd = env["ro"][RAY0:RAY0 + n], env["rd"][RAY0:RAY0 + n]
    rs = np.random.RandomState(5)
    noise2 = rs.rand(2, n, 64).astype(np.float32); bg2 = rs.rand(2, n, 3).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    inv_s = float(env["p"]["inv_s"])
    pa, pb = nsr_ops.render_rays_pair(env["f"], t(ro), t(rd), t(noise2), 64, 64, 1.6, inv_s, bg2=t(bg2), keep_weights=True)
    torch.cuda.synchronize()
    assert nsr_ops.handoff_timeouts(DEV) == 0
    for q, res in enumerate((pa, pb)):
        r = env["O"].render_rays(env["of"], ro, rd, 64, 64, 1.6, inv_s, bg=bg2[q], noise=noise2[q])
        for k in ("image", "weights_sum", "depth", "normal_map", "eik"):
            assert_bitwise(res[k], r[k], f"copy {q}: {k}")
        assert_bitwise(res["gradient_error"].reshape(1), np.float32([r["gradient_error"]]), f"copy {q}: gradient_error")
        if q == 1:
            for k in ("z_vals", "weights", "alpha", "color", "sdf", "gradient"):
                assert_bitwise(res[k], r[k], f"copy b: {k}")


def test_view_directions_ride_in_the_handoff_state(oracle):
    from avatarcraft_amd import nsr_ops
    from tests.test_oracle_viewdirs import viewdirs_field
    from tests.test_gpu_viewdirs import device_field_vd
    g = load_golden("viewdirs.npz")
    of, table = viewdirs_field(oracle, g)
    f = device_field_vd(g, table)
    ro, rd = make_rays(64, 64, dist=1.7, f=50.0)
    n = 520
    ro, rd = ro[RAY0:RAY0 + n], rd[RAY0:RAY0 + n]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    out = nsr_ops.render_rays(f, t(ro), t(rd), 64, 64, 1.6, float(g["inv_s"]), extras=True)
    torch.cuda.synchronize()
    assert nsr_ops.handoff_timeouts(DEV) == 0
    r = oracle.render_rays(of, ro, rd, 64, 64, 1.6, float(g["inv_s"]))
    for k in ("image", "weights_sum", "depth", "normal_map", "z_vals", "weights", "alpha", "color"):
        assert_bitwise(out[k], np.asarray(r[k]).reshape(tuple(out[k].shape)), k)


def test_back_to_back_launches_of_different_shapes(env):
    """2056 rays, 520 rays, 2056 again and 520 at 4 tiles, queued on one stream without a host synchronisation in between: each equals its launch alone
    (which the tests above hold to the oracle) -- the slot's cached lists are picked by shape, and a flag left by the previous launch never matches"""
    from avatarcraft_amd import nsr_ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    shapes = [(2056, 64, 64), (520, 64, 64), (2056, 64, 64), (520, 32, 32), (9, 64, 64), (2056, 64, 64)]
    alone = [_both(env, *s)[0] for s in shapes]
    rays = {n: (t(env["ro"][RAY0:RAY0 + n]), t(env["rd"][RAY0:RAY0 + n])) for n in (9, 520, 2056)}
    torch.cuda.synchronize()
    outs = [nsr_ops.render_rays(env["f"], rays[n][0], rays[n][1], T0, up, 1.6, float(env["p"]["inv_s"]), extras=True, debug_indices=True) for n, T0, up in shapes]
    torch.cuda.synchronize()
    assert nsr_ops.handoff_timeouts(DEV) == 0
    for s, a, o in zip(shapes, alone, outs):
        for k in FLOAT_KEYS + ["ss_inds", "sort_index", "gradient_error"]:
            assert torch.equal(a[k], o[k]), (s, k)
