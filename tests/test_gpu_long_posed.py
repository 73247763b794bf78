"""-m gpu: the long renderer in posed space (ac_render_rays_long_warped; nsr_ops.render_rays_long(warp=...), NeRFNetwork.posed_long_rays,
drivers.render_animation at long counts).  The CPU oracle's posed render stays inside the fused renderer's window, so the pins are:
  1. inside that window the two posed renderers agree bit for bit (the short one is pinned to the oracle bit for bit);
  2. at long and ragged counts an identity pose with every sample unmasked equals the canonical oracle bit for bit;
  3. the mask at long counts: the oracle's closest-face search on the kernel's mid points, alpha = oracle alpha * mask, and the compositing equal to
     the scan restatement that tests/test_long_posed_cpu.py validates against the oracle;
  4. a real pose against the reference's own run(render_can=False) at 128 + 128 and 100 + 64 (tests/golden/warp_render_long.npz);
  5. the model switch and the animation driver; 6. batching and the argument rules."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.common import load_golden, make_rays, make_body
from tests.gpu_common import device_field, oracle_field, assert_bitwise
from tests.test_long_posed_cpu import composite_scans, cube_near_far

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
RAY_KEYS = ["image", "weights_sum", "depth", "normal_map", "eik"]
SAMPLE_KEYS = ["z_vals", "weights", "alpha", "sdf", "color", "gradient"]


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@functools.lru_cache(maxsize=1)
def _env():
    from oracle import oracle as O
    from avatarcraft_amd import nsr_ops
    assert torch.cuda.is_available(), "these tests need a GPU"
    O.build()
    p = load_golden("nsr_params.npz")
    f, table = device_field(p)
    Wsh = t(np.random.RandomState(41).normal(0.0, 0.2, (64, 16)).astype(np.float32))
    fvd = nsr_ops.Field(f.t["table"], [int(v) for v in p["offsets"]], float(p["per_level_scale"]), 16, f.t["W1"], f.t["b1"], f.t["W2"], f.t["b2"],
                        f.t["Wc1"], f.t["Wc2"], f.t["Wc3"], Wc1_sh=Wsh)
    ro, rd = make_rays(20, 20, dist=1.8, f=17.0, jitter_seed=9)
    verts, faces, Ts = make_body()
    eye = np.tile(np.eye(4)[None], (Ts.shape[0], 1, 1))
    return dict(O=O, p=p, inv_s=float(p["inv_s"]), f=f, fvd=fvd, of=oracle_field(p, table), ro=ro, rd=rd, body=(verts, faces, Ts), eye=eye)


def _clone(g):
    return {k: v.clone() for k, v in g.items() if isinstance(v, torch.Tensor)}


# ------------------------------------------------------------------ 1. the short window: long posed == short posed, bit for bit
@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("guide", [True, False])
@pytest.mark.parametrize("T0,up", [(32, 32), (64, 64), (16, 0), (48, 80)])
def test_long_posed_equals_short_posed_bitwise(T0, up, guide, perturb, precision):
    from avatarcraft_amd import nsr_ops
    e = _env()
    ro, rd = t(e["ro"]), t(e["rd"])
    N, T = ro.shape[0], T0 + up
    wm = nsr_ops.WarpMesh(*e["body"], DEV, use_mesh_guide=guide)
    noise = t(np.random.RandomState(3).rand(N, T0)) if perturb else None
    bg = t(np.random.RandomState(5).uniform(0, 1, (N, 3)))
    for field in (e["f"], e["fvd"]):
        kw = dict(noise=noise, bg=bg, extras=True, debug_indices=True, warp=wm, precision=precision, cos_anneal_ratio=0.7)
        a = _clone(nsr_ops.render_rays(field, ro, rd, T0, up, 1.6, e["inv_s"], **kw))
        b = _clone(nsr_ops.render_rays_long(field, ro, rd, T0, up, 1.6, e["inv_s"], **kw))
        torch.cuda.synchronize()
        for k in RAY_KEYS + SAMPLE_KEYS + ["can_mid", "eik_res", "gradient_error"]:
            assert_bitwise(b[k], a[k].cpu().numpy(), k)
        assert torch.equal(a["mask"], b["mask"]) and b["mask"].shape == (N, T) and b["can_mid"].shape == (N, T, 3)
        assert bool(b["mask"].any()) and not bool(b["mask"].all()) and float(b["weights_sum"].max()) > 0.5
        if guide:
            assert torch.equal(a["near_m"], b["near_m"]) and torch.equal(a["far_m"], b["far_m"])
        if up:
            assert_bitwise(b["ss_inds"], a["ss_inds"].cpu().numpy(), "ss_inds")
            assert_bitwise(b["sort_index"], a["sort_index"][:, :, :T].cpu().numpy(), "sort_index")
        # skip_masked: the long renderer against the short one under the same option, and tests/test_gpu_render.py's rules against its own unskipped launch
        sa = _clone(nsr_ops.render_rays(field, ro, rd, T0, up, 1.6, e["inv_s"], skip_masked=True, **kw))
        sb = _clone(nsr_ops.render_rays_long(field, ro, rd, T0, up, 1.6, e["inv_s"], skip_masked=True, **kw))
        torch.cuda.synchronize()
        live = sb["mask"].bool()
        for k in RAY_KEYS + SAMPLE_KEYS + ["eik_res"]:
            assert_bitwise(sb[k], sa[k].cpu().numpy(), "skip_masked " + k)
        assert torch.equal(sa["mask"], sb["mask"]) and torch.equal(sa["can_mid"][live], sb["can_mid"][live])
        if "ray_dead" in sa:
            assert torch.equal(sa["ray_dead"], sb["ray_dead"])
        for k in ("image", "weights_sum", "depth", "normal_map", "weights", "alpha", "mask"):
            assert torch.equal(b[k], sb[k]), "skip_masked moved " + k
        lr = live.any(1)
        assert torch.equal(b["z_vals"][lr], sb["z_vals"][lr]) and torch.isfinite(sb["z_vals"]).all() and (sb["z_vals"][:, 1:] >= sb["z_vals"][:, :-1]).all()
        assert torch.equal(b["can_mid"][live], sb["can_mid"][live])
        assert torch.equal(b["sdf"][live], sb["sdf"][live]) and torch.equal(b["color"][live], sb["color"][live])
        if T % 16 == 0:
            dead = ~live.reshape(N, T // 16, 16).any(-1)
            assert bool(dead.any())
            assert float(sb["sdf"].reshape(N, T // 16, 16)[dead].abs().max()) == 0.0 and float(sb["color"].reshape(N, T // 16, 16, 3)[dead].abs().max()) == 0.0


# ------------------------------------------------------------------ 2. identity pose, every sample unmasked == the canonical oracle
@functools.lru_cache(maxsize=None)
def _identity_oracle(T0, up, guide):
    e = _env()
    verts = e["body"][0]
    nf = e["O"].mesh_near_far(e["ro"], e["rd"], verts, 0.05) if guide else None
    bg = np.random.RandomState(11).uniform(0, 1, (e["ro"].shape[0], 3)).astype(F32)
    return e["O"].render_rays(e["of"], e["ro"], e["rd"], T0, up, 1.6, e["inv_s"], bg=bg, near_far=nf), bg, nf


def _identity_render(T0, up, guide, threshold, **kw):
    from avatarcraft_amd import nsr_ops
    e = _env()
    verts, faces, _ = e["body"]
    _, bg, _ = _identity_oracle(T0, up, guide)
    wm = nsr_ops.WarpMesh(verts, faces, e["eye"], DEV, threshold, 0.05, use_mesh_guide=guide)
    g = _clone(nsr_ops.render_rays_long(e["f"], t(e["ro"]), t(e["rd"]), T0, up, 1.6, e["inv_s"], bg=t(bg), extras=True, warp=wm, **kw))
    torch.cuda.synchronize()
    return g


def _posed_mid_points(z, ro, rd):
    """o + d * zmid in fp32 (the render core's rule: z + 0.5 * delta, the last sample its own z), product then sum as the kernel forms them"""
    z = np.ascontiguousarray(z, F32)
    zmid = z.copy()
    zmid[:, :-1] = (z[:, :-1] + (F32(0.5) * (z[:, 1:] - z[:, :-1]).astype(F32)).astype(F32)).astype(F32)
    return (ro[:, None, :].astype(F32) + (rd[:, None, :].astype(F32) * zmid[:, :, None]).astype(F32)).astype(F32)


@pytest.mark.parametrize("T0,up,guide", [(100, 64, True), (128, 128, True), (50, 0, True), (17, 16, True), (256, 256, True), (2, 496, True), (100, 64, False)])
def test_identity_pose_equals_canonical_oracle_bitwise(T0, up, guide):
    e = _env()
    r, _, _ = _identity_oracle(T0, up, guide)
    g = _identity_render(T0, up, guide, 100.0)
    for k in RAY_KEYS + ["z_vals", "weights", "alpha", "sdf", "color"]:
        assert_bitwise(g[k], r[k], k)
    assert_bitwise(g["gradient_error"].reshape(1), np.float32([r["gradient_error"]]), "gradient_error")
    assert bool((g["mask"] == 1).all())
    assert_bitwise(g["can_mid"], _posed_mid_points(r["z_vals"], e["ro"], e["rd"]), "can_mid")
    assert r["weights_sum"].max() > 0.5


# ------------------------------------------------------------------ 3. the mask at long counts
@pytest.mark.parametrize("T0,up", [(100, 64), (128, 128)])
def test_mask_at_long_counts(T0, up):
    e = _env()
    verts, faces, _ = e["body"]
    N, T = e["ro"].shape[0], T0 + up
    r, bg, nf = _identity_oracle(T0, up, True)
    full = _identity_render(T0, up, True, 100.0)
    g = _identity_render(T0, up, True, 0.05)
    h = lambda k: g[k].cpu().numpy()
    assert_bitwise(g["z_vals"], full["z_vals"].cpu().numpy(), "z_vals")
    mask = h("mask").astype(bool)
    assert 0.02 < mask.mean() < 0.7
    assert np.array_equal(h("sdf").view(np.uint32)[mask], full["sdf"].cpu().numpy().view(np.uint32)[mask])
    assert np.array_equal(h("color").view(np.uint32)[mask], full["color"].cpu().numpy().view(np.uint32)[mask])
    mid = _posed_mid_points(h("z_vals"), e["ro"], e["rd"])
    omask = e["O"].warp_samples(mid.reshape(-1, 3), verts, faces, e["eye"], 0.05)[4].reshape(N, T)
    assert np.array_equal(mask, omask)
    assert_bitwise(g["alpha"], (r["alpha"] * omask.astype(F32)).astype(F32), "alpha = oracle alpha * mask")
    cn, cf = cube_near_far(e["ro"], e["rd"], 1.6)
    near, far = np.where(np.isinf(nf[0]), cn, nf[0]).astype(F32), np.where(np.isinf(nf[1]), cf, nf[1]).astype(F32)
    c = composite_scans(h("alpha"), h("color"), h("gradient"), h("z_vals"), near, far, bg)
    for k in ("weights", "image", "weights_sum", "depth", "normal_map"):
        assert_bitwise(g[k], c[k], "scan restatement: " + k)
    assert float(g["weights_sum"].max()) > 0.5 and float((g["weights_sum"] - full["weights_sum"]).abs().max()) > 1e-3       # the mask really gates alpha
    s = _identity_render(T0, up, True, 0.05, skip_masked=True)
    for k in ("image", "weights_sum", "depth", "normal_map", "weights", "alpha", "mask"):
        assert torch.equal(g[k], s[k]), "skip_masked moved " + k


# ------------------------------------------------------------------ 4. a real pose against the reference at long counts
MEDIAL_RAY = 0     # tests/test_oracle_golden.py: the ray on the symmetric body's medial axis (two faces equally close) is left out


@pytest.mark.parametrize("T0,up", [(128, 128), (100, 64)])
def test_long_posed_vs_reference_golden(T0, up):
    """Bounds: on rays whose sample positions agree with the reference's within 1e-4 the project's acceptance bound 1e-3 for image / weights_sum / depth and
    the existing posed check's 1e-2 (normal_map) and 2e-3 (alpha, weights); on rays where an up-sampling or closest-face knife edge moved the later
    samples the existing check's 2e-2 for the pixel; such rays at most 12 % of the 256 (the reference against the oracle's arithmetic with its count
    check widened gives 20 and 22 rays at these counts); gradient_error within 5e-4 (the same comparison gives 2.4e-4 and 9.6e-5)."""
    from avatarcraft_amd import nsr_ops
    e = _env()
    gd = load_golden("warp_render_long.npz")
    tag = f"{T0}_{up}"
    wm = nsr_ops.WarpMesh(*e["body"], DEV, use_mesh_guide=True)
    g = nsr_ops.render_rays_long(e["f"], t(gd["rays_o"]), t(gd["rays_d"]), T0, up, 1.6, e["inv_s"], bg=t(gd["bg"]), extras=True, warp=wm)
    torch.cuda.synchronize()
    n = gd["rays_o"].shape[0]
    keep = np.ones(n, bool); keep[MEDIAL_RAY] = False
    d = lambda k: np.abs(g[k].cpu().numpy().reshape(gd[f"{tag}_{k}"].shape) - gd[f"{tag}_{k}"]).reshape(n, -1).max(1)
    zbad = d("z_vals") > 1e-4
    ok, flip = keep & ~zbad, keep & zbad
    ge = abs(float(g["gradient_error"]) - float(gd[f"{tag}_gradient_error"]))
    note = dict(counts=tag, flipped=np.nonzero(flip)[0].tolist(), agreeing={k: float(d(k)[ok].max()) for k in ("image", "weights_sum", "depth", "normal_map", "alpha", "weights")},
                flipped_image=float(d("image")[flip].max(initial=0)), gradient_error=ge)
    assert d("image")[ok].max() <= 1e-3 and d("weights_sum")[ok].max() <= 1e-3 and d("depth")[ok].max() <= 1e-3, note
    assert d("normal_map")[ok].max() <= 1e-2, note
    assert d("alpha")[ok].max() <= 2e-3 and d("weights")[ok].max() <= 2e-3, note
    assert d("image")[flip].max(initial=0) <= 2e-2, note
    assert int(flip.sum()) <= 0.12 * n, note
    assert ge <= 5e-4, note
    assert gd[f"{tag}_weights_sum"].max() > 0.5


# ------------------------------------------------------------------ 5. model and driver
def test_model_switch():
    from avatarcraft_amd import nsr_ops
    from tests.test_gpu_model import golden_net
    net, _ = golden_net()
    net.eval()
    e = _env()
    ro, rd = t(e["ro"]), t(e["rd"])
    wm = nsr_ops.WarpMesh(*e["body"], DEV, use_mesh_guide=True)
    kw = dict(num_steps=128, bound=1.6, upsample_steps=128, staged=False, render_can=False, verts=wm, perturb=False, cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0)
    assert net.posed_long_rays is False
    with torch.no_grad(), pytest.raises(NotImplementedError, match="posed-space rendering supports"):
        net.render(ro[None], rd[None], **kw)
    net.posed_long_rays = True
    try:
        with torch.no_grad():
            out = net.render(ro[None], rd[None], **kw)
            lean = net.render(ro[None], rd[None], per_sample=False, **kw)
            ref = nsr_ops.render_rays_long(net._field(), ro, rd, 128, 128, 1.6, net.forward_variance(), extras=True, warp=wm, precision=net.render_precision)
        torch.cuda.synchronize()
        for a, b in (("rgb", "image"), ("depth", "depth"), ("weight_sum", "weights_sum"), ("normal", "normal_map"), ("weights", "weights"), ("pts_alpha", "alpha"),
                     ("z_vals", "z_vals"), ("pts_color", "color"), ("gradient_error", "gradient_error")):
            assert torch.equal(out[a].reshape(ref[b].shape), ref[b]), a
        assert torch.equal(lean["rgb"], out["rgb"]) and lean["weights"] is None
        assert out["z_vals"].shape == (ro.shape[0], 256) and float(out["weight_sum"].max()) > 0.5
        for prm in net.parameters():
            prm.requires_grad_(True)
        with pytest.raises(NotImplementedError, match="short window"):
            net.render(ro[None], rd[None], **kw)
    finally:
        net.posed_long_rays = False


def test_render_animation_at_long_counts():
    """two frames at 100 + 64; the driver's view is its 512-pixel camera at an integer stride, so 64 x 64 (48 does not divide 512)"""
    from avatarcraft_amd import drivers as DR, smpl as SM, nsr_ops
    from avatarcraft_amd.render_utils import NSR_BOUND
    from tests.test_gpu_model import golden_net
    net, _ = golden_net()
    net.eval()
    verts, faces, _ = make_body()
    bm = SM.BodyModel.synthetic(seed=2, n_verts=verts.shape[0], faces=faces, v_template=verts)
    cam = np.eye(4, dtype=np.float32); cam[:3, 3] = [0.0, 0.0, 2.2]
    poses = (np.random.RandomState(1).normal(size=(2, 72)) * 0.2).astype(np.float32)
    res = 64
    assert net.posed_long_rays is False and net.skip_masked_samples is False and net.warp_temporal_seeds is True
    frames = list(DR.render_animation(net, bm, cam, poses=poses, resolution=res, max_frames=2, num_steps=100, upsample_steps=64))
    assert net.posed_long_rays is False and net.skip_masked_samples is False
    assert len(frames) == 2 and frames[0][1].shape == (res, res, 3)
    world_verts, Ts, n_frames = SM.calc_local_trans(bm, render_type="animate", poses=poses, max_frames=2)
    ro, rd = DR.gen_rays_pose(cam, 512 // res, device=DEV)
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    with torch.no_grad():
        for i in range(2):
            wm = nsr_ops.WarpMesh(world_verts[i], np.asarray(bm.faces), Ts[i], DEV)
            ref = nsr_ops.render_rays_long(net._field(), ro, rd, 100, 64, NSR_BOUND, net.forward_variance(), warp=wm, precision=net.render_precision)
            torch.cuda.synchronize()
            assert torch.equal(frames[i][1].reshape(-1, 3), ref["image"]), i
    assert float((frames[0][1] - frames[1][1]).abs().max()) > 1e-3 and float((frames[0][1] < 0.99).float().mean()) > 0.02
    # a generator abandoned after its first frame restores the switch too
    it = DR.render_animation(net, bm, cam, poses=poses, resolution=res, max_frames=2, num_steps=100, upsample_steps=64)
    next(it); it.close()
    assert net.posed_long_rays is False and net.skip_masked_samples is False


# ------------------------------------------------------------------ 6. batching and rules
def test_whole_frame_in_one_batch():
    from avatarcraft_amd import nsr_ops
    e = _env()
    verts, faces, Ts = make_body(n_lat=83, n_lon=83)
    ro, rd = make_rays(256, 256, dist=1.8, f=0.78125 * 256)
    ro_t, rd_t = t(ro), t(rd)
    wm = nsr_ops.WarpMesh(verts, faces, Ts, DEV, use_mesh_guide=True)
    for skip in (False, True):
        parts = []
        for i in range(0, 65536, 8192):
            o = nsr_ops.render_rays_long(e["f"], ro_t[i:i + 8192], rd_t[i:i + 8192], 128, 128, 1.6, e["inv_s"], warp=wm, skip_masked=skip)
            parts.append({k: o[k].clone() for k in ("image", "depth", "weights_sum")})
        big = nsr_ops.render_rays_long(e["f"], ro_t, rd_t, 128, 128, 1.6, e["inv_s"], warp=wm, skip_masked=skip)
        torch.cuda.synchronize()
        for k in ("image", "depth", "weights_sum"):
            assert torch.equal(big[k], torch.cat([q[k] for q in parts])), (k, skip)
        assert 0.05 < float((big["weights_sum"] > 0.5).float().mean()) < 0.6
        del big, parts
    nsr_ops.free_scratch()


def test_phase_marks_of_both_posed_entries():
    """ac_debug_warped_phases: both posed entries mark the six boundaries of the one posed sequence; the hook changes no value"""
    from avatarcraft_amd import nsr_ops, _lib as L
    e = _env()
    ro, rd = t(e["ro"][200:216]), t(e["rd"][200:216])              # (16 rays of the middle row of the 20 x 20 view: they cross the body)
    wm = nsr_ops.WarpMesh(*e["body"], DEV, use_mesh_guide=True)
    calls = [lambda: nsr_ops.render_rays(e["f"], ro, rd, 32, 32, 1.6, e["inv_s"], extras=True, warp=wm),
             lambda: nsr_ops.render_rays_long(e["f"], ro, rd, 20, 16, 1.6, e["inv_s"], extras=True, warp=wm)]     # (20: a count only the long kernel takes)
    plain = [_clone(c()) for c in calls]
    torch.cuda.synchronize()
    L.lib().ac_debug_warped_phases(1)
    try:
        for c, ref in zip(calls, plain):
            got = _clone(c())
            ph = (C.c_float * 5)(*([-1.0] * 5))
            assert L.lib().ac_debug_warped_phase_ms(C.addressof(ph)) == 0
            assert all(np.isfinite(v) and v >= 0.0 for v in ph), list(ph)
            torch.cuda.synchronize()
            for k in RAY_KEYS + SAMPLE_KEYS + ["can_mid", "eik_res"]:
                assert_bitwise(got[k], ref[k].cpu().numpy(), k)
            assert torch.equal(got["mask"], ref["mask"])
    finally:
        L.lib().ac_debug_warped_phases(0)
    assert float(plain[0]["weights_sum"].max()) > 0.5 and plain[1]["z_vals"].shape == (16, 36)


def test_rules():
    from avatarcraft_amd import nsr_ops, _lib as L
    e = _env()
    wm = nsr_ops.WarpMesh(*e["body"], DEV)
    ro, rd = make_rays(4, 4)
    ro, rd = t(ro), t(rd)
    for T0, up, rule in ((400, 128, "<= 512"), (64, 40, "multiple of 16"), (1, 16, "num_steps >= 2")):
        with pytest.raises(RuntimeError, match=rule):
            nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, 1.0, warp=wm)
    with pytest.raises(RuntimeError, match="opacity_only"):
        nsr_ops.render_rays_long(e["f"], ro, rd, 100, 64, 1.6, 1.0, warp=wm, opacity_only=True)
    with pytest.raises(RuntimeError):
        nsr_ops.render_rays_long(e["f"], ro.cpu(), rd, 100, 64, 1.6, 1.0, warp=wm)
    out = nsr_ops.render_rays_long(e["f"], ro[:0], rd[:0], 100, 64, 1.6, 1.0, warp=wm, extras=True)
    assert out["image"].shape == (0, 3) and out["z_vals"].shape == (0, 164) and out["mask"].shape == (0, 164) and out["can_mid"].shape == (0, 164, 3)
    # the raw entry: feat7, opacity_only, a bad count, an empty mesh and a short scratch are refused with the rule in the message
    lz, lu = nsr_ops.linspace_tables(100, torch.device(DEV))
    o = L.ac_render_out()
    keep = [torch.empty(64, device=DEV) for _ in range(5)]
    for k, b in zip(("image", "weights_sum", "depth", "normal_map", "eik"), keep):
        setattr(o, k, b.data_ptr())
    nbytes = L.lib().ac_render_rays_warped_scratch(16, 164, None)
    sc = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)

    def call(op, out=o, mesh=wm.c, scratch_bytes=int(nbytes)):
        return L.lib().ac_render_rays_long_warped(C.byref(e["f"].c), C.byref(op), ro.data_ptr(), rd.data_ptr(), None, None, lz.data_ptr(), lu.data_ptr(),
                                                  C.byref(mesh), sc.data_ptr(), scratch_bytes, C.byref(out), None)
    mk = lambda ns=100, us=64, opacity=0: L.ac_render_opts(16, ns, us, 1.6, 1.0, 1.0, 0.005, 0, None, None, None, 0, 0, opacity)
    assert call(mk(), scratch_bytes=1024) != 0 and b"scratch" in L.lib().ac_last_error()
    assert call(mk(opacity=1)) != 0 and b"opacity_only" in L.lib().ac_last_error()
    assert call(mk(400, 128)) != 0 and b"<= 512" in L.lib().ac_last_error()
    assert call(mk(100, 40)) != 0 and b"multiple of 16" in L.lib().ac_last_error()
    o7 = L.ac_render_out()
    for k, b in zip(("image", "weights_sum", "depth", "normal_map", "eik"), keep):
        setattr(o7, k, b.data_ptr())
    o7.feat7 = keep[0].data_ptr()
    assert call(mk(), out=o7) != 0 and b"feat7" in L.lib().ac_last_error()
    empty = L.ac_warp_mesh()
    assert call(mk(), mesh=empty) != 0 and b"mesh" in L.lib().ac_last_error()
    assert call(mk()) == 0
    torch.cuda.synchronize()
    # the canonical entry keeps refusing the posed-space option
    with pytest.raises(RuntimeError, match="posed-space option"):
        nsr_ops.render_rays_long(e["f"], ro, rd, 100, 64, 1.6, 1.0, skip_masked=True)
