"""CPU tier of the long posed renderer (ac_render_rays_long_warped; GPU tier: tests/test_gpu_long_posed.py).

The CPU oracle's posed render stays inside the fused renderer's window (orc_render_rays_warped), so the GPU tier pins the masked compositing at long
counts against a restatement of the two documented scans (Kogge-Stone offsets 1, 2, 4, 8 inside tiles of 16 samples, a sequential
carry between tiles, a ragged last tile padded with the identity).  That restatement -- composite_scans below, numpy fp32 -- is validated here first:
fed the oracle's own per-sample outputs of a canonical 100 + 64 render it must return the oracle's per-ray outputs bit for bit."""
import os
import re

import numpy as np

from tests.common import make_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def cube_near_far(ro, rd, bound):
    """near_far_from_bound (cube) in fp32, the renderers' arithmetic (ac_devmath.hpp: cube_near_far)"""
    ro, rd, b = np.asarray(ro, F32), np.asarray(rd, F32), F32(bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = rd + F32(1e-15)
        a, c = (-b - ro) / e, (b - ro) / e
    lo, hi = np.where(a < c, a, c), np.where(a > c, a, c)
    near = lo[:, 0].copy()
    for k in (1, 2):
        near = np.where(lo[:, k] > near, lo[:, k], near)
    far = hi[:, 0].copy()
    for k in (1, 2):
        far = np.where(hi[:, k] < far, hi[:, k], far)
    near = np.where(near < F32(0.05), F32(0.05), near)
    return near.astype(F32), far.astype(F32)


def _row_scan(v, mul):
    """Kogge-Stone inclusive scan over the last axis (16 lanes): offsets 1, 2, 4, 8; lanes below the offset take the identity"""
    ident = F32(1.0) if mul else F32(0.0)
    v = v.astype(F32).copy()
    for off in (1, 2, 4, 8):
        s = np.full_like(v, ident)
        s[..., off:] = v[..., :-off]
        v = (s * v if mul else s + v).astype(F32)
    return v


def composite_scans(alpha, color, gradient, z_vals, near, far, bg=None):
    """the render core's compositing from per-sample alpha [N,T], colour [N,T,3], finite-difference gradient [N,T,3] and z [N,T] (all fp32), inside
    the range near / far [N]: -> weights [N,T], image [N,3], weights_sum [N], depth [N], normal_map [N,3], every operation in fp32 in the kernels' order"""
    alpha, color, gradient, z = (np.ascontiguousarray(a, F32) for a in (alpha, color, gradient, z_vals))
    N, T = alpha.shape
    nt = (T + 15) // 16
    pad = nt * 16 - T
    gn = np.sqrt((gradient[..., 0] * gradient[..., 0] + gradient[..., 1] * gradient[..., 1]) + gradient[..., 2] * gradient[..., 2]).astype(F32)
    normal = (gradient / (F32(1e-5) + gn)[..., None]).astype(F32)
    span = (np.asarray(far, F32) - np.asarray(near, F32)).astype(F32)
    zn01 = np.clip(((z - np.asarray(near, F32)[:, None]) / span[:, None]).astype(F32), F32(0.0), F32(1.0))
    om = (F32(1.0) - alpha + F32(1e-7)).astype(F32)

    def tiles(a, fill):
        return np.concatenate([a, np.full((N, pad) + a.shape[2:], fill, F32)], 1).reshape((N, nt, 16) + a.shape[2:]) if pad else a.reshape((N, nt, 16) + a.shape[2:])
    om_t, al_t = tiles(om, 1.0), tiles(alpha, 0.0)
    weights = np.zeros((N, nt, 16), F32)
    cT = np.ones(N, F32)
    for c in range(nt):
        loc = _row_scan(om_t[:, c], True)
        sh = np.ones_like(loc)
        sh[:, 1:] = loc[:, :-1]
        tex = sh if c == 0 else (cT[:, None] * sh).astype(F32)
        tex[:, 0] = F32(1.0) if c == 0 else cT
        cT = loc[:, 15] if c == 0 else (cT * loc[:, 15]).astype(F32)
        weights[:, c] = (al_t[:, c] * tex).astype(F32)

    def total(term):                                            # [N, nt, 16] -> [N]: tile totals of the add scan, summed over the tiles in order
        acc = None
        for c in range(nt):
            t = _row_scan(term[:, c], False)[:, 15]
            acc = t if c == 0 else (acc + t).astype(F32)
        return acc
    col_t, nrm_t, zn_t = tiles(color, 0.0), tiles(normal, 0.0), tiles(zn01, 0.0)
    s_w = total(weights)
    s_c = np.stack([total((col_t[..., k] * weights).astype(F32)) for k in range(3)], 1)
    s_n = np.stack([total((nrm_t[..., k] * weights).astype(F32)) for k in range(3)], 1)
    s_d = total((weights * zn_t).astype(F32))
    b = np.ones((N, 3), F32) if bg is None else np.asarray(bg, F32).reshape(N, 3)
    image = (s_c + ((F32(1.0) - s_w)[:, None] * b).astype(F32)).astype(F32)
    return dict(weights=weights.reshape(N, nt * 16)[:, :T], image=image, weights_sum=s_w, depth=s_d, normal_map=s_n)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_scan_restatement_reproduces_the_oracle_bitwise():
    """a ragged count (164 samples: ten full tiles and four lanes of an eleventh), inside an explicit near / far range and inside the cube's own"""
    from oracle import oracle as O
    from tests.common import oracle_field_from_golden, load_golden
    O.build()
    p = load_golden("nsr_params.npz")
    of = oracle_field_from_golden(p)
    ro, rd = make_rays(8, 8, dist=1.7, f=6.0, jitter_seed=4)
    N = ro.shape[0]
    bg = np.random.RandomState(7).uniform(0, 1, (N, 3)).astype(F32)
    cn, cf = cube_near_far(ro, rd, 1.6)
    for near_far in ((cn + F32(0.15), cf - F32(0.2)), None):
        r = O.render_rays(of, ro, rd, 100, 64, 1.6, float(p["inv_s"]), bg=bg, near_far=near_far)
        near, far = (cn, cf) if near_far is None else near_far
        assert np.array_equal(_bits(r["z_vals"][:, 0]), _bits(near)), "the first coarse sample sits on near: the range is the one the oracle used"
        c = composite_scans(r["alpha"], r["color"], r["gradient"], r["z_vals"], near, far, bg)
        for k in ("image", "weights_sum", "depth", "weights", "normal_map"):
            assert np.array_equal(_bits(c[k]), _bits(r[k])), (k, float(np.abs(c[k] - r[k]).max()))
        assert r["weights_sum"].max() > 0.5 and r["weights_sum"].min() < 0.05


def test_long_posed_entry_is_declared_and_opt_in():
    """the C entry is part of the header and of the ctypes table; the model's switch exists and is off by default; the Python rules that need no device"""
    import pytest
    from avatarcraft_amd import _lib, nsr_ops
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    hdr = open(os.path.join(ROOT, "include", "avatarcraft_hip.h")).read()
    assert re.search(r"\bint ac_render_rays_long_warped\s*\(", hdr) and "ac_render_rays_long_warped" in _lib.EXPORTS
    assert NeRFNetwork.posed_long_rays is False and NeRFNetwork.skip_masked_samples is False
    import inspect
    assert inspect.signature(nsr_ops.render_rays_long).parameters["warp"].default is None
    import torch
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="posed-space option"):
        nsr_ops.render_rays_long(None, z, z, 100, 64, skip_masked=True)
    with pytest.raises(RuntimeError, match="opacity_only"):
        nsr_ops.render_rays_long(None, z, z, 100, 64, warp=object(), opacity_only=True)
    with pytest.raises(RuntimeError, match="<= 512"):
        nsr_ops.render_rays_long(None, z, z, 400, 128, warp=object())
