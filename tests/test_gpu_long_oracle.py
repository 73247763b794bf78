"""-m gpu: the long renderer (ac_render_rays_long / ac_sample_rays_long) against the CPU oracle, bit for bit, over its whole envelope (num_steps >= 2,
upsample_steps a multiple of 16, at most 512 samples).  The counts exercise what the long renderer does and the fused one does not
(render_long.hip): a masked last coarse tile (a few valid lanes), a masked last render tile, one-bin first up-sampling passes, 31 passes with the
sharpness 64 * 2^30, and T = 512 (the LDS slab's capacity).  The oracle is pinned to the reference at these counts by tests/test_oracle_long.py."""
import functools
import json

import numpy as np
import pytest
import torch

from tests.common import load_golden, make_rays, edge_case_rays
from tests.gpu_common import device_field, oracle_field, assert_bitwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

COUNTS = [(2, 0), (2, 16), (2, 496),              # one-bin first up-sample; 31 passes
          (17, 0), (17, 48), (37, 0), (43, 32),   # one or a few valid lanes in the last coarse tile; 5 and 11 in the last render tile
          (100, 64), (241, 256),                  # ragged coarse and render tiles
          (128, 128), (32, 480), (16, 496),       # T = 512
          (256, 0), (497, 0)]
MODES = ["eval", "perturb", "near_far", "viewdirs"]
CASES = [(T0, up, mode, prec) for T0, up in COUNTS for mode in MODES for prec in ("exact", "fast")]
BIG_CASES = [(T0, up, prec) for T0, up in ((100, 64), (241, 256)) for prec in ("exact", "fast")]
FLOAT_KEYS = ["image", "weights_sum", "depth", "normal_map", "eik", "z_vals", "weights", "alpha", "color", "sdf", "gradient"]
# fast precision: test_gpu_render.py's split (test_render_full_baseline_view_vs_oracle) -- the sample positions, indices and sdf bit for bit; the
# quantities the split-bf16 finite differences move within its bounds.  alpha depends on the normal through iter_cos * delta * inv_s, so the same
# normal difference moves a pixel in proportion to the section length: without up-sampling and below 32 samples the bounds grow by 32 / T (2 + 0:
# x16, measured 9.2e-5 in a pixel, 2.0e-4 in weights_sum); every other count here holds the 64 + 64 view's bounds.
FAST_EXACT_KEYS = ["z_vals", "sdf"]
FAST_BOUNDS = (("image", 2e-5), ("weights_sum", 2e-5), ("normal_map", 5e-5), ("weights", 2e-5), ("color", 2e-5))


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@functools.lru_cache(maxsize=1)
def _env():
    from oracle import oracle as O
    from tests.test_gpu_viewdirs import device_field_vd
    from tests.test_oracle_viewdirs import viewdirs_field
    O.build()
    p = load_golden("nsr_params.npz")
    f, table = device_field(p)
    gv = load_golden("viewdirs.npz")
    ofv, tablev = viewdirs_field(O, gv)
    ro, rd = make_rays(12, 12, dist=1.7, f=9.0, jitter_seed=2)
    ero, erd = edge_case_rays()
    return dict(O=O, inv_s=float(p["inv_s"]), f=f, of=oracle_field(p, table), fvd=device_field_vd(gv, tablev), ofvd=ofv, inv_s_vd=float(gv["inv_s"]),
                ro=np.concatenate([ro, ero]), rd=np.concatenate([rd, erd]))


def _near_far(ro, rd):
    """tests/test_gpu_long_rays.py's range: a sub-interval of the cube's on most rays, +-inf (keep the cube's) on every fifth"""
    from tests.test_gpu_long_rays import _near_far as nf
    n, f = nf(ro, rd)
    return n.cpu().numpy(), f.cpu().numpy()


def _inputs(T0, up, mode, big=False):
    e = _env()
    if big:
        ro, rd = make_rays(37, 27, dist=1.7, f=12.0, jitter_seed=5)      # 999 rays: not a multiple of the 7 waves or the 8 XCDs rays are dealt to
    else:
        ro, rd = e["ro"], e["rd"]
    N = ro.shape[0]
    rs = np.random.RandomState(T0 * 1000 + up)
    kw = dict(bg=rs.uniform(0, 1, (N, 3)).astype(np.float32), cos_anneal_ratio=1.0, noise=None, near_far=None)
    if mode == "perturb":
        kw.update(noise=rs.uniform(0, 1, (N, T0)).astype(np.float32), cos_anneal_ratio=0.7)
    if mode == "near_far":
        kw["near_far"] = _near_far(ro, rd)
    if mode == "viewdirs":
        kw["cos_anneal_ratio"] = 0.4
        return ro, rd, kw, e["fvd"], e["ofvd"], e["inv_s_vd"]
    return ro, rd, kw, e["f"], e["of"], e["inv_s"]


@functools.lru_cache(maxsize=1)
def _oracle(T0, up, mode, big=False):
    """one oracle render per (count, mode), shared by both precisions (the cases run in that order)"""
    ro, rd, kw, _, of, inv_s = _inputs(T0, up, mode, big)
    return _env()["O"].render_rays(of, ro, rd, T0, up, 1.6, inv_s, **kw)


def _check(T0, up, mode, precision, big=False):
    from avatarcraft_amd import nsr_ops
    ro, rd, kw, f, _, inv_s = _inputs(T0, up, mode, big)
    r = _oracle(T0, up, mode, big)
    T, nup = T0 + up, up // 16
    nf = None if kw["near_far"] is None else (t(kw["near_far"][0]), t(kw["near_far"][1]))
    g = nsr_ops.render_rays_long(f, t(ro), t(rd), T0, up, 1.6, inv_s, bg=t(kw["bg"]), noise=t(kw["noise"]), near_far=nf,
                                 cos_anneal_ratio=kw["cos_anneal_ratio"], extras=True, debug_indices=True, precision=precision)
    z = nsr_ops.sample_rays_long(f, t(ro), t(rd), T0, up, 1.6, noise=t(kw["noise"]), near_far=nf)
    torch.cuda.synchronize()
    for k in (FLOAT_KEYS if precision == "exact" else FAST_EXACT_KEYS):
        assert_bitwise(g[k], r[k], k)
    assert_bitwise(z, r["z_vals"], "sample_rays_long z_vals")
    if nup:
        assert_bitwise(g["ss_inds"], r["ss_inds"], "ss_inds")
        assert_bitwise(g["sort_index"], r["sort_index"][:, :nup, :T], "sort_index")
    if precision == "exact":
        assert_bitwise(g["gradient_error"].reshape(1), np.float32([r["gradient_error"]]), "gradient_error")
    else:
        worst = {k: float(np.abs(g[k].cpu().numpy() - r[k]).max()) for k, _ in FAST_BOUNDS}
        print(json.dumps({f"fast_{T0}_{up}_{mode}{'_999' if big else ''}": worst}))
        scale = 32.0 / T if up == 0 and T < 32 else 1.0
        for k, tol in FAST_BOUNDS:
            assert worst[k] <= tol * scale, (k, worst)


@pytest.mark.parametrize("T0,up,mode,precision", CASES)
def test_long_renderer_equals_oracle(T0, up, mode, precision):
    _check(T0, up, mode, precision)


@pytest.mark.parametrize("T0,up,precision", BIG_CASES)
def test_long_renderer_equals_oracle_999_rays(T0, up, precision):
    _check(T0, up, "eval", precision, big=True)
