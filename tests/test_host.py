"""CPU: host-side logic and the C-ABI library (loads, exports every symbol of include/avatarcraft_hip.h;
no compute calls without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.common import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from avatarcraft_amd import build as hb, _lib
    hb.build()
    hdr = open(os.path.join(ROOT, "include", "avatarcraft_hip.h")).read()
    declared = set(re.findall(r"\b(ac_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"ac_field", "ac_render_opts", "ac_render_out"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = _lib.lib()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.ac_version() == 10
    # host helper needs no GPU: level table == oracle's == SURVEY Appendix B
    scale = (ctypes.c_float * 16)(); res = (ctypes.c_uint32 * 16)()
    S = float(np.float32(np.log2(1.381912879967776)))
    lib.ac_hash_level_table(16, S, 16, ctypes.cast(scale, ctypes.c_void_p), ctypes.cast(res, ctypes.c_void_p))
    from oracle import oracle as O
    so, ro = O.hash_level_table(16, np.float32(S), 16)
    assert list(scale) == so.tolist() and list(res) == ro.tolist() and scale[15] == 2047.0


def test_struct_layout_matches_header():
    from avatarcraft_amd import _lib
    assert ctypes.sizeof(_lib.ac_render_opts) == 72 and _lib.ac_render_opts.opacity_only.offset == 64 and _lib.ac_render_opts.precision.offset == 56 and _lib.ac_render_opts.inv_s_dev.offset == 32 and _lib.ac_render_opts.far_m.offset == 48
    assert ctypes.sizeof(_lib.ac_render_out) == 17 * 8 and _lib.ac_render_out.sdf_out16.offset == 13 * 8 and _lib.ac_render_out.feat7.offset == 15 * 8
    assert ctypes.sizeof(_lib.ac_core_saved) == 10 * 8 and ctypes.sizeof(_lib.ac_core_upstream) == 6 * 8 and ctypes.sizeof(_lib.ac_core_grads) == 7 * 8 and _lib.ac_core_grads.split_level.offset == 5 * 8 and _lib.ac_core_grads.g_sh_tiles.offset == 6 * 8
    assert ctypes.sizeof(_lib.ac_adam_entry) == 40 and _lib.ac_adam_entry.n.offset == 32 and _lib.AC_ADAM_MAX_TENSORS == 16
    assert ctypes.sizeof(_lib.ac_wn_layer) == 40 and _lib.ac_wn_layer.rows.offset == 24 and ctypes.sizeof(_lib.ac_pg_entry) == 56 and _lib.ac_pg_entry.kind.offset == 52
    assert _lib.ac_field.offsets.offset == 8 and _lib.ac_field.S.offset == 8 + 17 * 4 and _lib.ac_field.W1.offset == 88 and _lib.ac_field.prepared.offset == 88 + 7 * 8 and _lib.ac_field.Wc1_sh.offset == 88 + 8 * 8 and ctypes.sizeof(_lib.ac_field) == 88 + 9 * 8


def test_packed_param_grad_layout_matches_header():
    """nsr_ops.split_sdf_param_grads / split_color_param_grads against the layouts as include/avatarcraft_hip.h words them, in literals:
    g_sdf_params [3344] = dW1 [64][36] (column 35 = db1) | dW2 [16][64] | db2 [16];
    g_color_params [7168] = dWc1 [64][32] (columns 0..20) | dWc2 [64][64] | dWc3 [16][64] (rows 0..2).  Needs neither the library nor a GPU."""
    from avatarcraft_amd import nsr_ops
    assert (nsr_ops.SDF_PARAM_GRADS_LEN, nsr_ops.COLOR_PARAM_GRADS_LEN) == (3344, 7168)
    r, c = torch.arange(64.)[:, None], torch.arange(64.)[None, :]
    g = torch.arange(3344.)
    W1, b1, W2, b2 = nsr_ops.split_sdf_param_grads(g)
    assert [tuple(t.shape) for t in (W1, b1, W2, b2)] == [(64, 35), (64,), (16, 64), (16,)]
    assert torch.equal(W1, 36 * r + c[:, :35]) and torch.equal(b1, 36 * r[:, 0] + 35)
    assert torch.equal(W2, 2304 + 64 * r[:16] + c) and torch.equal(b2, 3328 + r[:16, 0])
    assert [t.data_ptr() - g.data_ptr() for t in (W1, b1, W2, b2)] == [0, 4 * 35, 4 * 2304, 4 * 3328]
    k = torch.arange(7168.)
    Wc1, Wc2, Wc3 = nsr_ops.split_color_param_grads(k)
    assert [tuple(t.shape) for t in (Wc1, Wc2, Wc3)] == [(64, 21), (64, 64), (3, 64)]
    assert torch.equal(Wc1, 32 * r + c[:, :21]) and torch.equal(Wc2, 2048 + 64 * r + c) and torch.equal(Wc3, 6144 + 64 * r[:3] + c)
    assert [t.data_ptr() - k.data_ptr() for t in (Wc1, Wc2, Wc3)] == [0, 4 * 2048, 4 * 6144]
    for t, base in ((W1, g), (b1, g), (W2, g), (b2, g), (Wc1, k), (Wc2, k), (Wc3, k)):         # views: same storage, and a write shows in the vector
        assert t.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
    W2[3, 5] = -1.0
    assert g[2304 + 64 * 3 + 5] == -1.0
    # the table the no-autograd step hands to ac_param_grads as (offset, row stride) says the same
    S, K = nsr_ops.SDF_PARAM_GRADS, nsr_ops.COLOR_PARAM_GRADS
    assert [(S[n].offset, S[n].stride) for n in ("W1", "b1", "W2", "b2")] == [(0, 36), (35, 36), (2304, 64), (3328, 1)]
    assert [(K[n].offset, K[n].stride) for n in ("Wc1", "Wc2", "Wc3")] == [(0, 32), (2048, 64), (6144, 64)]
    with pytest.raises(RuntimeError, match="3344"):
        nsr_ops.split_sdf_param_grads(torch.zeros(7168))


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from avatarcraft_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_ops_reject_cpu_tensors():
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.encoder.hashencoder.backend import _backend
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        nsr_ops._chk(torch.zeros(3, 3), "x")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        _backend.hash_encode_forward(torch.zeros(1, 3), torch.zeros(4, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 1, 2),
                                     1, 3, 2, 1, 1.0, 2, False, torch.zeros(1))


def test_encoder_surface_matches_reference_facts():
    """get_encoder / HashEncoder bookkeeping against facts recorded from the reference's Python (encoder_facts.npz)."""
    from avatarcraft_amd.encoder import get_encoder
    g = load_golden("encoder_facts.npz")
    cfgs = {"default": dict(hash_num_levels=16, hash_level_dim=2, hash_per_level_scale=1.3819, hash_base_resolution=16,
                            hash_log2_hashmap_size=19, hash_desired_resolution=2048),
            "small": dict(hash_num_levels=8, hash_level_dim=4, hash_per_level_scale=2.0, hash_base_resolution=4,
                          hash_log2_hashmap_size=12, hash_desired_resolution=None)}
    for tag, cfg in cfgs.items():
        enc, dim = get_encoder("hashgrid", dict(in_dim=3, **cfg))
        assert np.array_equal(enc.offsets.numpy(), g[f"{tag}_offsets"]) and dim == int(g[f"{tag}_dim"])
        assert float(enc.per_level_scale) == float(g[f"{tag}_pls"]) and int(enc.n_params) == int(g[f"{tag}_nparams"])
        assert enc.embeddings.shape == (int(g[f"{tag}_offsets"][-1]), cfg["hash_level_dim"])
        assert float(enc.embeddings.abs().max()) <= 1e-4
    fe, fdim = get_encoder("frequency", dict(in_dim=3, freq_multires=6))
    assert fdim == int(g["freq_dim"])
    assert np.array_equal(fe(torch.from_numpy(g["freq_in"])).numpy(), g["freq_out"])
    sh, shdim = get_encoder("sh", dict(in_dim=3))
    assert shdim == 16
    with pytest.raises(NotImplementedError):
        get_encoder("tiled", {})


def test_bench_refuses_to_run_without_gpu():
    import subprocess, sys
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in (r.stderr + r.stdout)


def test_dropin_registers_reference_module_names():
    import sys
    import avatarcraft_amd.dropin as d
    names = d.install()
    try:
        import encoder, raymarching                      # noqa: F401  (the reference's top-level names)
        from encoder import get_encoder
        from encoder.hashencoder import HashEncoder
        from encoder.shencoder import SHEncoder
        from encoder.hashencoder.backend import _backend as hb
        from raymarching.backend import _backend as rb
        assert HashEncoder.__module__.startswith("avatarcraft_amd") and SHEncoder.__module__.startswith("avatarcraft_amd")
        for fn in ("hash_encode_forward", "hash_encode_backward"):
            assert hasattr(hb, fn)
        for fn in ("march_rays_train", "composite_rays_train_forward", "composite_rays_train_backward", "march_rays",
                   "composite_rays", "compact_rays"):
            assert hasattr(rb, fn)
        for fn in ("march_rays_train", "composite_rays_train", "march_rays", "composite_rays", "compact_rays"):
            assert hasattr(raymarching, fn)
        assert "encoder.freq_encoder" in names
    finally:
        d.uninstall()
    assert "encoder" not in sys.modules


# ------------------------------------------------------------------ SMPL skinning (row a14)
def test_smpl_lbs_matches_reference_golden():
    import torch
    from avatarcraft_amd import smpl as SM
    g = load_golden("smpl.npz")
    bm = SM.BodyModel.synthetic(seed=3, n_verts=600)
    pose, betas = torch.from_numpy(g["pose"]), torch.from_numpy(g["betas"])
    R = SM.batch_rodrigues(pose.view(-1, 3))
    assert np.abs(R.numpy() - g["R"]).max() < 1e-6
    assert np.abs(R[1].numpy() - np.eye(3)).max() < 1e-6             # the zero rotation
    T, v, dv = SM.lbs(betas, pose, *bm._args(), return_T=True, concat_joints=True)
    assert T.shape == (1, 624, 4, 4) and v.shape == (1, 624, 3)
    assert np.abs(T.numpy() - g["T"]).max() < 2e-6 and np.abs(v.numpy() - g["v"]).max() < 1e-6 and np.abs(dv.numpy() - g["dv"]).max() < 1e-6
    verts, joints = SM.lbs(betas, pose, *bm._args())
    assert np.abs(verts.numpy() - g["verts"]).max() < 2e-6 and np.abs(joints.numpy() - g["joints"]).max() < 2e-6
    # the entry points: numpy in, numpy out
    vv, TT, _ = bm.verts_transformations(g["pose"], g["betas"], return_tensor=False, concat_joints=True)
    assert TT.shape == (624, 4, 4) and np.abs(TT - g["T"][0]).max() < 2e-6
    vt, _, _ = bm.verts_transformations(g["pose"], g["betas"], transl=np.array([[0.1, 0.2, 0.3]], np.float32), return_tensor=False)
    assert vt.shape == (600, 3)


def test_calc_local_trans_properties():
    """render_warp.py:127-222 needs the licensed pickle, so the composition is pinned by its invariants: the da pose with zero
    betas is the rest pose => T_rest2pose = I (Ts = I / 0.9) and the world vertices are the rest-pose vertices."""
    from avatarcraft_amd import smpl as SM
    bm = SM.BodyModel.synthetic(seed=5, n_verts=300)
    g = np.random.default_rng(0)
    poses = np.concatenate([SM.da_pose(), (g.standard_normal((2, 72)) * 0.3).astype(np.float32)], 0)
    wv, Ts, n = SM.calc_local_trans(bm, poses=poses, max_frames=3)
    assert n == 3 and Ts[0].shape == (324, 4, 4) and Ts[0].dtype == np.float64 and wv[0].shape == (300, 3) and wv[0].dtype == np.float32
    assert np.abs(Ts[0] * SM.SMPL_SCALE - np.eye(4)[None]).max() < 1e-5
    rest = bm.forward(SM.da_pose(), np.zeros((1, 10), np.float32), return_tensor=False)
    assert np.abs(wv[0] - rest).max() < 1e-5
    # a posed frame: applying Ts*0.9 to the rest vertices gives the world vertices; the rigid part stays a rotation blend
    rest_h = np.concatenate([rest, np.ones((300, 1), np.float32)], 1)
    assert np.abs(np.einsum("vij,vj->vi", Ts[1][:300] * SM.SMPL_SCALE, rest_h)[:, :3] - wv[1]).max() < 1e-5
    # shape interpolation: n_interp frames, zero pose
    wv2, Ts2, n2 = SM.calc_local_trans(bm, render_type="interp_shape", shape_from=np.zeros((1, 10)), shape_to=np.ones((1, 10)), n_interp=4)
    assert n2 == 4 and np.isfinite(Ts2[3]).all() and np.abs(wv2[0] - wv2[3]).max() > 1e-4
    with pytest.raises(NotImplementedError):
        SM.calc_local_trans(bm, render_type="other")


def test_calc_local_trans_matches_reference_golden(tmp_path):
    """render_warp.calc_local_trans (render_warp.py:127-222) run by tests/golden/make_golden.py on a synthetic SMPL_NEUTRAL.pkl
    (BodyModel.synthetic(5) in the licensed file's layout): Ts [V+24,4,4] fp64 and world_verts, animation / shape interpolation / scale"""
    from avatarcraft_amd import smpl as SM
    g = load_golden("local_trans.npz")
    bm = SM.BodyModel.synthetic(seed=5)
    keep = g["keep"]
    for tag, kw in (("anim", dict(render_type="animate", poses=g["poses"], shape_from=g["shape_from"], shape_to=g["shape_to"])),
                    ("shape", dict(render_type="interp_shape", shape_from=g["shape_from"], shape_to=g["shape_to"], n_interp=4, max_frames=3)),
                    ("scaled", dict(scale=1.25, render_type="animate", poses=g["poses"][1:2]))):
        wv, Ts, n = SM.calc_local_trans(bm, **kw)
        if f"{tag}_n" in g:
            assert n == int(g[f"{tag}_n"])
        assert Ts[0].dtype == np.float64 and Ts[0].shape == (6914, 4, 4) and wv[0].dtype == np.float32 and wv[0].shape == (6890, 3)
        assert np.abs(np.stack(Ts)[:, keep] - g[f"{tag}_Ts"]).max() < 5e-6
        assert np.abs(np.stack(wv)[:, ::53] - g[f"{tag}_world_verts"]).max() < 5e-6
    # the same through the pickle reader (the layout of the licensed file: posedirs [V,3,207], kintree_table, uint32(-1) root parent)
    import pickle
    kt = np.stack([np.array(SM.SMPL_PARENTS, np.int64), np.arange(24, dtype=np.int64)]); kt[0, 0] = 2 ** 32 - 1
    d = dict(f=np.asarray(bm.faces, np.uint32), v_template=bm.v_template.numpy(), shapedirs=bm.shapedirs.numpy(),
             posedirs=bm.posedirs.numpy().T.reshape(6890, 3, -1), J_regressor=bm.J_regressor.numpy(), kintree_table=kt, weights=bm.lbs_weights.numpy())
    os.makedirs(tmp_path / "smpl")
    with open(tmp_path / "smpl" / "SMPL_NEUTRAL.pkl", "wb") as f:
        pickle.dump(d, f, protocol=2)
    bm2 = SM.BodyModel.from_pickle(str(tmp_path / "smpl"))
    wv2, Ts2, _ = SM.calc_local_trans(bm2, render_type="animate", poses=g["poses"][2:3])
    assert np.abs(Ts2[0][keep] - g["anim_Ts"][2]).max() < 5e-6
    with pytest.raises(FileNotFoundError):
        SM.BodyModel.from_pickle(str(tmp_path / "nowhere"))


def test_convert_amass_matches_reference_script(tmp_path):
    """utils/convert_amass.py:1-19 run by make_golden.py on a synthetic AMASS-layout archive (poses [47,156], betas [16])"""
    from avatarcraft_amd import smpl as SM
    g = load_golden("local_trans.npz")
    np.savez(tmp_path / "seq.npz", poses=g["amass_poses"], betas=g["amass_betas"])
    poses, betas = SM.convert_amass(str(tmp_path / "seq.npz"))
    assert poses.dtype == np.float32 and np.array_equal(poses, g["amass_out"])
    assert np.array_equal(betas, g["amass_betas"][:10]) and (poses[:, 21:] == 0).all()
    SM.save_pose_sequence(tmp_path / "seq.pkl", poses)
    seq = SM.load_pose_sequence(tmp_path / "seq.pkl")
    assert seq.shape == (5, 72) and np.array_equal(seq.reshape(5, 24, 3), poses)
    bm = SM.BodyModel.synthetic(seed=5, n_verts=200)
    wv, Ts, n = SM.calc_local_trans(bm, render_type="animate", poses=seq, max_frames=2)             # what render_warp.py --poseseq_path does next
    assert n == 2 and Ts[1].shape == (224, 4, 4)


# ------------------------------------------------------------------ config-1 plumbing (row a19)
def test_vanilla_nerf_plumbing_matches_reference():
    """BASELINE config 1: 64x64 rays, 16 samples, PE(10)/PE(4), NeRF 8x256 with view directions, white background -- against the
    reference's own models/nerf.py + ray_to_samples + raw2outputs (tests/golden/vanilla.npz), CPU like the reference"""
    import torch
    from avatarcraft_amd import nerf as NF
    from avatarcraft_amd.encoder import get_encoder
    g, r = load_golden("vanilla.npz"), load_golden("rays.npz")
    pe, pdim = get_encoder("frequency", dict(in_dim=3, freq_multires=10))
    de, ddim = get_encoder("frequency", dict(in_dim=3, freq_multires=4))
    assert (pdim, ddim) == (63, 27)
    torch.manual_seed(0)
    net = NF.NeRF(depth=8, width=256, input_ch=pdim, input_ch_views=ddim, use_viewdirs=True)        # same RNG stream as the reference's ctor
    assert sum(p.numel() for p in net.parameters()) == int(g["n_params"])
    ro, rd = torch.from_numpy(r["kat64_o"]), torch.from_numpy(r["kat64_d"])
    with torch.no_grad():
        rgb, disp, acc, w, depth = NF.render_rays_vanilla(net, pe, de, ro, rd, 1.0, 4.0, 16)
    assert rgb.shape == (4096, 3) and w.shape == (4096, 16)
    for name, val in (("rgb", rgb), ("disp", disp), ("acc", acc), ("weights", w), ("depth", depth)):
        v, ref = val.numpy(), g[name]
        assert np.array_equal(np.isnan(v), np.isnan(ref)), name            # disp = 1/max(1e-10, depth/acc) is NaN where acc == 0 (0/0), as in the reference
        ok = ~np.isnan(ref)
        tol = 1e-4 if name == "disp" else 2e-6        # disp = 1 / (depth / acc) amplifies the last bits of two sums where acc is tiny (2.4e-5 between two hosts' BLAS)
        assert np.abs(v[ok] - ref[ok]).max() <= tol * max(1.0, np.abs(ref[ok]).max()), name
    batch = dict(origin=ro, direction=rd, near=torch.full((4096, 1), 1.0), far=torch.full((4096, 1), 4.0))
    pts, dirs, z = NF.ray_to_samples(batch, 16)
    assert np.array_equal(z.numpy(), g["z"]) and pts.shape == (4096, 16, 3) and dirs.shape == (4096, 16, 3)
    torch.manual_seed(3)
    _, _, zp = NF.ray_to_samples(batch, 16, perturb=1.0)
    assert np.array_equal(zp.numpy(), g["z_perturbed"])                                                # same draw order and clipping
    # the no-viewdirs / skip / tanh-scale variant with the reference's weights loaded by name
    net2 = NF.NeRF(depth=4, width=32, input_ch=pdim, output_ch=4, skips=[1], scale=0.5, scale_type='tanh')
    net2.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("net2.")}, strict=True)
    with torch.no_grad():
        raw2 = net2(pe(pts.reshape(-1, 3)[:64]))
    assert np.abs(raw2.numpy() - g["raw2"]).max() <= 1e-6


# ------------------------------------------------------------------ training views of the stylize outer loop
def test_style_paths_match_reference():
    """style_360_path (front / back sectors, head close-ups), describe_view and the camera jitter of pose_spherical against the
    reference under the same numpy seed (tests/golden/paths.npz)"""
    from avatarcraft_amd import render_utils as RU
    g = load_golden("paths.npz")
    c, up = np.array([0.0, 0.1, 0.0]), np.array([0.0, 1.0, 0.0])
    poses, desc = RU.style_360_path(c, up, 1.8, 20)
    assert np.abs(np.stack([p.camera_to_world for p in poses]) - g["plain_c2w"]).max() < 1e-6 and list(desc) == list(g["plain_desc"])
    np.random.seed(7)
    poses, desc = RU.style_360_path(c, up, 1.8, 20, add_noise=True, noise_scale=2.0, style_head=True, head_offset=0.423, head_rate=0.4, head_dist=0.45)
    assert len(poses) == 20 + 8 and list(desc) == list(g["noisy_desc"]) and desc[-1].startswith("front view of the face")
    assert np.abs(np.stack([p.camera_to_world for p in poses]) - g["noisy_c2w"]).max() < 1e-6
    np.random.seed(9)
    poses, _ = RU.default_360_path(c, up, 1.8, 8, add_noise=True)
    assert np.abs(np.stack([p.camera_to_world for p in poses]) - g["ring_noisy_c2w"]).max() < 1e-6


def test_dataset_camera_rays_match_reference():
    """gen_rays_pose (the camera of render_warp.py) against utils/SMPLDataset.py:86-103 (tests/golden/dataset_rays.npz)"""
    from avatarcraft_amd.drivers import gen_rays_pose
    g = load_golden("dataset_rays.npz")
    o, v = gen_rays_pose(g["pose"], 8, device="cpu")
    assert o.shape == (64, 64, 3) and np.array_equal(o.numpy(), g["rays_o"]) and np.abs(v.numpy() - g["rays_d"]).max() <= 1e-7


# ------------------------------------------------------------------ SDS guidance (row a18)
def test_sds_guidance_matches_reference_over_stub_models():
    """avatarcraft_amd.guidance.StableDiffusion against the reference's models/diffusion.py:StableDiffusion, both over the same tiny seeded
    VAE / UNet / tokenizer / text encoder (tests/common_sd.py; tests/golden/sds.npz was recorded by importing the reference over stub
    `diffusers` / `transformers` modules): text embeddings, the noise schedule, and the image gradient of mannual_backward for two image
    sizes and timesteps"""
    from avatarcraft_amd.guidance import StableDiffusion, SDSGuidance
    from tests import common_sd as SD
    g = load_golden("sds.npz")
    sd = StableDiffusion(torch.device("cpu"), "1.5", components=SD.components())
    emb = sd.get_text_embeds(["Hulk, photorealistic style"])
    assert emb.shape == (2, 77, 16) and np.array_equal(emb.numpy(), g["text_embeds"])
    assert np.abs(sd.alphas.numpy()[::50] - g["alphas_cumprod"]).max() < 1e-7
    assert (sd.min_step, sd.max_step) == (20, 980)
    for seed in (11, 12):
        pred = torch.from_numpy(g[f"rgb_{seed}"]).clone().requires_grad_(True)
        torch.manual_seed(seed)
        sd.mannual_backward(emb, pred, 100)
        assert pred.grad.shape == pred.shape
        assert np.abs(pred.grad.numpy() - g[f"grad_{seed}"]).max() <= 2e-4 * np.abs(g[f"grad_{seed}"]).max()      # 5e-5 between two hosts' oneDNN convolutions
        torch.manual_seed(seed)
        gr = SDSGuidance(sd, "Hulk, photorealistic style", 100.0)(torch.from_numpy(g[f"rgb_{seed}"]))       # the callable sds_step takes
        assert np.abs(gr.numpy() - g[f"grad_{seed}"]).max() <= 2e-4 * np.abs(g[f"grad_{seed}"]).max() and not gr.requires_grad
    # the guidance changes with the prompt and with the scale; without diffusers the default constructor says what is missing
    torch.manual_seed(11)
    other = SDSGuidance(sd, "a wooden statue", 100.0)(torch.from_numpy(g["rgb_11"]))
    assert float((other - torch.from_numpy(g["grad_11"])).abs().max()) > 1e-4
    try:
        import diffusers  # noqa: F401
    except Exception:
        with pytest.raises(RuntimeError, match="diffusers"):
            StableDiffusion(torch.device("cpu"), "1.5")
    with pytest.raises(ValueError):
        StableDiffusion(torch.device("cpu"), "3.0", components=SD.components())


def test_dropin_fused_route_serves_models_instant_nsr(tmp_path, monkeypatch):
    """dropin.install(fused=True): inside the reference's own `models` package the module `instant_nsr` -- and nothing else -- comes from this package, through
    every import form the reference's drivers use (render_canonical.py:30 `import models.instant_nsr as instant_nsr`, stylize.py:17 `from models import
    instant_nsr, diffusion`); a stand-in `models` package plays the reference's"""
    import sys
    import avatarcraft_amd.dropin as d
    pkg = tmp_path / "models"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "instant_nsr.py").write_text("WHO = 'reference'\n")
    (pkg / "diffusion.py").write_text("WHO = 'reference'\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        monkeypatch.delitem(sys.modules, k)
    d.install(fused=True)
    try:
        import models.instant_nsr as a
        from models import instant_nsr as b, diffusion
        import models
        assert a is b is models.instant_nsr and a.__name__ == "avatarcraft_amd.instant_nsr" and hasattr(a, "NeRFNetwork")
        assert diffusion.WHO == "reference"
    finally:
        d.uninstall()
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
    import importlib
    importlib.invalidate_caches()
    import models.instant_nsr as c
    assert c.WHO == "reference"                      # after uninstall the package serves its own module again
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        del sys.modules[k]


def test_dtype_codes_and_adam_argument_checks():
    """host-side checks that need no GPU: the dtype dispatch of the encoders (the reference's CHECK_IS_FLOATING / one scalar_t per call) and the one-launch
    Adam's refusal of tensors it cannot step"""
    from avatarcraft_amd import _lib
    from avatarcraft_amd.stylize import Adam
    assert _lib.dtype_code(torch.zeros(1)) == 0 and _lib.dtype_code(torch.zeros(1, dtype=torch.float16)) == 1 and _lib.dtype_code(torch.zeros(1, dtype=torch.float64)) == 2
    with pytest.raises(RuntimeError, match="floating tensor"):
        _lib.dtype_code(torch.zeros(1, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="floating tensor"):
        _lib.dtype_code(torch.zeros(1, dtype=torch.int32), "grad")
    with pytest.raises(RuntimeError, match="must have the dtype of inputs"):
        _lib.dtype_code(torch.zeros(1, dtype=torch.float16), "inputs", ((torch.zeros(1), "embeddings"),))
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    opt = Adam([p], lr=1e-3, zero_grad_in_step=True)
    with pytest.raises(RuntimeError, match="CUDA"):
        opt.step()                                           # a CPU parameter: no silent fallback to torch's update
    assert float(p.abs().max()) == 0.0 and not opt.grads_cleared
    opt.zero_grad()
    assert opt.grads_cleared and p.grad is not None and float(p.grad.abs().max()) == 0.0      # cleared in place, never dropped
    p.grad.add_(1.0)                                         # anything that writes a gradient afterwards withdraws the claim (version counters, not a sticky flag)
    assert not opt.grads_cleared
    opt.zero_grad(); assert opt.grads_cleared
    (p * 2.0).sum().backward()
    assert not opt.grads_cleared and float(p.grad.min()) == 2.0
    assert set(opt.state_dict()["param_groups"][0].keys()) == set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3).state_dict()["param_groups"][0].keys())


def test_drivers_shard_views_round_robin_over_ranks():
    """multi-GPU inference: views / frames are dealt to the ranks round robin, every index exactly once, no collective"""
    from avatarcraft_amd.drivers import shard_indices
    assert shard_indices(10) == list(range(10))                        # no process group: everything
    parts = [shard_indices(10, r, 4) for r in range(4)]
    assert parts == [[0, 4, 8], [1, 5, 9], [2, 6], [3, 7]]
    assert sorted(i for p_ in parts for i in p_) == list(range(10))
    assert shard_indices(3, 5, 8) == [] and shard_indices(0, 0, 1) == []
    with pytest.raises(ValueError):
        shard_indices(4, 2, 2)


def test_header_is_self_contained_c_and_a_c_program_links_against_the_library(tmp_path):
    """the drop-in boundary is a C ABI: include/avatarcraft_hip.h must compile on its own as C99 and as C++ (round 6 found it leaning on the includer for size_t),
    and a plain C program that includes nothing else must link against libavatarcraft_hip.so and reach its host-side entry points"""
    import subprocess
    from avatarcraft_amd import build as hb, _lib
    hb.build()
    hdr = os.path.join(ROOT, "include", "avatarcraft_hip.h")
    subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-pedantic", "-std=c99", "-x", "c", hdr], check=True)
    subprocess.run(["g++", "-fsyntax-only", "-Wall", "-x", "c++", hdr], check=True)
    src = tmp_path / "abi.c"
    src.write_text('#include "avatarcraft_hip.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '    float scale[16]; uint32_t res[16];\n'
                   '    ac_hash_level_table(16, 0.46668363f, 16, scale, res);\n'
                   '    ac_field f; ac_render_opts o; ac_warp_mesh m; ac_core_upstream u;\n'
                   '    printf("%d %d %u %zu %zu %zu %zu %zu\\n", ac_version(), (int)scale[15], res[0], sizeof f, sizeof o, sizeof m, sizeof u, ac_sdf_stencil_backward_scratch(0));\n'
                   '    return ac_last_error()[0] != 0;\n}\n')
    exe = tmp_path / "abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), _lib.LIB_PATH, f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    out = r.stdout.split()
    assert out[0] == "10" and out[1] == "2047" and out[2] == "16"
    assert [int(v) for v in out[3:7]] == [ctypes.sizeof(_lib.ac_field), ctypes.sizeof(_lib.ac_render_opts), ctypes.sizeof(_lib.ac_warp_mesh), ctypes.sizeof(_lib.ac_core_upstream)]
