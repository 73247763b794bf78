"""-m gpu: rendering from the half-precision hash table (ac_table_to_half, ac_render_rays_h16, ac_render_rays_warped_h16).

The contract (include/avatarcraft_hip.h): a render from the half table equals, bit for bit and in every output, the fp32 entry's render of the widened
table T16 = table.half().float() -- and so, in exact precision, the CPU oracle's render of T16.  CPU tier: tests/test_half_table_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.common import load_golden, make_rays, make_body, edge_case_rays
from tests.gpu_common import device_field, oracle_field, assert_bitwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOAT_KEYS = ["image", "weights_sum", "depth", "normal_map", "eik", "z_vals", "weights", "alpha", "color", "sdf", "gradient"]
LEAN_KEYS = ["image", "weights_sum", "depth", "normal_map", "eik", "eik_res"]


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def widened(table):
    return torch.from_numpy(np.ascontiguousarray(table, np.float32)).half().float().numpy()


def field_like(f, table):
    """the Field f with another table"""
    from avatarcraft_amd import nsr_ops
    offs = [int(v) for v in f.c.offsets]
    g = nsr_ops.Field(t(table), offs, 2.0 ** f.S, f.H, f.t["W1"], f.t["b1"], f.t["W2"], f.t["b2"], f.t["Wc1"], f.t["Wc2"], f.t["Wc3"],
                      Wc1_sh=f.t.get("Wc1_sh"))
    g.S = f.S
    g.c.S = f.c.S                                                      # (the level scale's own bits, not a round trip through 2 ** S)
    return g


@pytest.fixture(scope="module")
def env(oracle):
    assert torch.cuda.is_available(), "these tests need a GPU"
    p = load_golden("nsr_params.npz")
    f, table = device_field(p)
    t16 = widened(table)
    fw = field_like(f, t16)
    return dict(p=p, f=f, fw=fw, table=table, of16=oracle_field(p, t16), O=oracle, inv_s=float(p["inv_s"]))


def same_bits(a, b, keys, what=""):
    for k in keys:
        x, y = a[k], b[k]
        if x.dtype.is_floating_point:
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, k, float((x - y).abs().max()))
        else:
            assert torch.equal(x, y), (what, k)


def all_keys(up):
    return FLOAT_KEYS + ["eik_res"] + (["ss_inds", "sort_index"] if up else [])


# ------------------------------------------------------------------ 1. conversion
def test_table_to_half_equals_torch_half_and_counts_overflows(env):
    from avatarcraft_amd import _lib as L, nsr_ops
    n = 1000003
    rs = np.random.RandomState(11)
    tab = (rs.standard_normal((n, 2)) * 10.0 ** rs.uniform(-9, 5.2, (n, 2))).astype(np.float32)       # subnormal halves up to beyond 65504
    hand = [0.0, -0.0, 6e-8, 5.9e-5, 6.2e-5, 65504.0, 65519.9, 65520.0, 1e6, np.inf, -np.inf, np.nan, -65520.0, -1e6,
            1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -25, -(1.0 + 2.0 ** -11), 2.0 ** -14 - 2.0 ** -25,
            1e-45, 65504.0 + 15.9]                                                                     # halfway cases: ties go to the even half
    hv = np.float32(hand)
    tab[:len(hv), 0] = hv
    tab[100:100 + len(hv), 1] = hv
    tab[200:200 + len(hv), 0] = hv; tab[200:200 + len(hv), 1] = hv[::-1]
    x = torch.from_numpy(tab).to(DEV)
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    conv = lambda: L.check(L.lib().ac_table_to_half(x.data_ptr(), n, out.data_ptr(), n_bad.data_ptr(), L.current_stream(x.device)), "table_to_half")
    conv()
    torch.cuda.synchronize()
    want = x.half()
    got = out.view(torch.float16).view(n, 2)                                   # little endian: channel 0 in the low half of the dword
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) == 4
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    assert int(((want == 0) & (x != 0)).sum()) > 1000 and int(((want.float().abs() < 6.1e-5) & (want != 0)).sum()) > 1000      # underflow and subnormals occur
    bad = (torch.isinf(want) & torch.isfinite(x)).any(dim=1)
    assert int(bad.sum()) > 1000 and int(n_bad.item()) == int(bad.sum())
    conv()                                                                     # n_bad is accumulated into
    assert int(n_bad.item()) == 2 * int(bad.sum())
    # a field that does not fit fp16 must not render silently
    big = env["table"].copy()
    big[12345, 1] = 1e6
    fb = field_like(env["f"], big)
    with pytest.raises(RuntimeError, match="1 of .* beyond the fp16 range"):
        fb.half_table()
    ro, rd = make_rays(4, 4)
    with pytest.raises(RuntimeError, match="beyond the fp16 range"):
        nsr_ops.render_rays(fb, t(ro), t(rd), 64, 64, 1.6, env["inv_s"], table_dtype="half")
    h = env["f"].half_table()
    assert h.dtype == torch.int32 and h.shape == (env["table"].shape[0],) and env["f"].half_table() is h      # made once per Field
    assert torch.equal(h.view(torch.float16).view(-1, 2).view(torch.int16), env["f"].t["table"].half().view(torch.int16))


# ------------------------------------------------------------------ 2. exact precision == the oracle on T16
def _oracle_cases():
    g = {n: load_golden(f"run_{n}.npz") for n in ("eval_64_64", "eval_32_32", "eval_64_0", "train_64_64")}
    cases = {n: (d["rays_o"], d["rays_d"], int(d["num_steps"]), int(d["upsample_steps"]), d["bg"], d.get("noise")) for n, d in g.items()}
    e = g["eval_64_64"]
    cases["eval_16_0"] = (e["rays_o"], e["rays_d"], 16, 0, e["bg"], None)
    cases["eval_16_112"] = (e["rays_o"], e["rays_d"], 16, 112, e["bg"], None)
    return cases


def _check_oracle(env, f, of, ro, rd, T0, up, bg, noise):
    from avatarcraft_amd import nsr_ops
    g = nsr_ops.render_rays(f, t(ro), t(rd), T0, up, 1.6, env["inv_s"], bg=t(bg), noise=t(noise), extras=True, debug_indices=True, table_dtype="half")
    lean = nsr_ops.render_rays(f, t(ro), t(rd), T0, up, 1.6, env["inv_s"], bg=t(bg), noise=t(noise), table_dtype="half")
    torch.cuda.synchronize()
    r = env["O"].render_rays(of, ro, rd, T0, up, 1.6, env["inv_s"], bg=bg, noise=noise)
    for k in FLOAT_KEYS:
        assert_bitwise(g[k], r[k], k)
    if up:
        assert_bitwise(g["ss_inds"], r["ss_inds"], "ss_inds")
        assert_bitwise(g["sort_index"], r["sort_index"], "sort_index")
    assert_bitwise(g["gradient_error"].reshape(1), np.float32([r["gradient_error"]]), "gradient_error")
    assert "z_vals" not in lean
    for k in ("image", "weights_sum", "depth", "normal_map", "eik"):
        assert_bitwise(lean[k], r[k], "lean " + k)
    assert_bitwise(lean["gradient_error"].reshape(1), np.float32([r["gradient_error"]]), "lean gradient_error")
    assert float(np.asarray(r["weights_sum"]).max()) > 0.5


@pytest.mark.parametrize("name", ["eval_64_64", "eval_32_32", "eval_64_0", "train_64_64", "eval_16_0", "eval_16_112"])
def test_half_render_equals_the_oracle_on_the_widened_table(env, name):
    _check_oracle(env, env["f"], env["of16"], *_oracle_cases()[name])


def test_half_render_with_view_directions_equals_the_oracle(env):
    from tests.test_oracle_viewdirs import viewdirs_field
    from tests.test_gpu_viewdirs import device_field_vd
    g = load_golden("viewdirs.npz")
    of, table = viewdirs_field(env["O"], g)
    of16 = env["O"].Field(widened(table), g["offsets"], g["W1"], g["b1"], g["W2"], g["b2"], g["Wc1"], g["Wc2"], g["Wc3"], float(g["per_level_scale"]))
    f = device_field_vd(g, table)
    assert f.has_viewdirs
    e = dict(env, inv_s=float(g["inv_s"]))
    _check_oracle(e, f, of16, g["rays_o"], g["rays_d"], 64, 64, g["bg"], None)
    _check_oracle(e, f, of16, g["rays_o"], g["rays_d"], 64, 64, g["bg"], g["train_noise"])


# ------------------------------------------------------------------ 3. both precisions == the fp32 entry on T16
def _pair(env, fh, fw, ro, rd, T0, up, precision, lean=False, **kw):
    """(the half-table render of field fh, the fp32 render of fw = fh with the widened table)"""
    from avatarcraft_amd import nsr_ops
    ex = {} if lean else dict(extras=True, debug_indices=True)
    a = nsr_ops.render_rays(fh, ro, rd, T0, up, 1.6, env["inv_s"], precision=precision, table_dtype="half", **ex, **kw)
    b = nsr_ops.render_rays(fw, ro, rd, T0, up, 1.6, env["inv_s"], precision=precision, **ex, **kw)
    torch.cuda.synchronize()
    return a, b


@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("n", [1, 63, 513, 4100])
def test_half_render_equals_fp32_render_of_the_widened_table(env, n, precision):
    """batch sizes across the 512-ray chunk, the 8-XCD wrap and the 4-segment hand-off"""
    ro, rd = make_rays(65, 64, dist=1.7, f=50.0)
    ro, rd = t(ro[:n]), t(rd[:n])
    a, b = _pair(env, env["f"], env["fw"], ro, rd, 64, 64, precision)
    same_bits(a, b, all_keys(64), f"n={n}")
    a, b = _pair(env, env["f"], env["fw"], ro, rd, 64, 64, precision, lean=True)
    same_bits(a, b, LEAN_KEYS, f"lean n={n}")
    if n >= 63:
        assert float(a["weights_sum"].max()) > 0.5 and float(a["weights_sum"].min()) < 0.05


# ------------------------------------------------------------------ 4. edges of the table
@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_half_render_at_the_edges_of_the_table(env, precision):
    """rays that miss the cube, graze a face or run along an edge outside it (their points clamp to +-bound: the top cell of every level), a near / far
    override -- on a field whose LAST entry of every level carries a value of its own: a descriptor sized in the wrong unit turns entries into zeros
    (or a neighbouring level's), which shows as a wrong feature here, not as a fault"""
    offs = [int(v) for v in env["p"]["offsets"]]
    tab = env["table"].copy()
    for l in range(16):
        tab[offs[l + 1] - 1] = (0.25 + 0.0625 * l, -0.125 - 0.03125 * l)         # exact in fp16
        tab[offs[l]] = (-0.375, 0.5)
    fh, fw = field_like(env["f"], tab), field_like(env["f"], widened(tab))
    ro, rd = edge_case_rays()
    ro2 = np.float32([[1.7, 1.7, -2.0], [1.7, 1.7, 2.0], [-1.7, 1.65, -2.0], [1.6, 1.6, -2.0], [2.0, 2.0, 2.0], [-2.0, -2.0, -2.0]])
    rd2 = np.float32([[0, 0, 1], [0, 0, -1], [0, 0, 1], [0, 0, 1], [-0.57735026, -0.57735026, -0.57735026], [0.57735026, 0.57735026, 0.57735026]])
    ro, rd = np.concatenate([ro, ro2]), np.concatenate([rd, rd2])
    N = ro.shape[0]
    for T0, up in ((64, 64), (16, 16)):
        a, b = _pair(env, fh, fw, t(ro), t(rd), T0, up, precision)
        same_bits(a, b, all_keys(up), "edge rays")
        nf = (torch.full((N,), 0.4, device=DEV), torch.full((N,), 3.6, device=DEV))      # the edge runners now end exactly on the corner (+-1.6, 1.6, 1.6)
        a, b = _pair(env, fh, fw, t(ro), t(rd), T0, up, precision, near_far=nf)
        same_bits(a, b, all_keys(up), "near_far override")
    # the distinctive entries are seen: the same rays on the unmarked field give other features
    c, _ = _pair(env, env["f"], env["fw"], t(ro), t(rd), 16, 16, precision, near_far=nf)
    assert not torch.equal(a["sdf"], c["sdf"])


# ------------------------------------------------------------------ 5. posed space
@pytest.mark.parametrize("guide", [True, False])
@pytest.mark.parametrize("T0,up", [(32, 32), (16, 16)])
def test_half_posed_render_equals_fp32_posed_render_of_the_widened_table(env, T0, up, guide):
    from avatarcraft_amd import nsr_ops
    verts, faces, Ts = make_body()
    ro, rd = make_rays(16, 16, dist=1.8, f=13.6, jitter_seed=9)
    ro, rd = t(ro), t(rd)
    N = ro.shape[0]
    keys = all_keys(up) + ["mask", "can_mid"]
    for precision in ("exact", "fast"):
        for skip in (False, True):
            for seeds in (False, True):
                res = []
                for half in (True, False):
                    wm = nsr_ops.WarpMesh(verts, faces, Ts, DEV, use_mesh_guide=guide)
                    if seeds:                                               # temporal seeds: each side starts from its own (equal) buffer
                        wm.bind_seeds(nsr_ops.WarpMesh.new_seed_buffer(N, T0 + T0 + up, DEV))
                    o = None
                    for _frame in range(2 if seeds else 1):                 # (the second frame starts from the faces the first one found)
                        o = nsr_ops.render_rays(env["f"] if half else env["fw"], ro, rd, T0, up, 1.6, env["inv_s"], extras=True, debug_indices=True, warp=wm,
                                                skip_masked=skip, precision=precision, table_dtype="half" if half else "float")
                    torch.cuda.synchronize()
                    res.append({k: v.clone() for k, v in o.items() if isinstance(v, torch.Tensor)})
                a, b = res
                what = f"{precision} skip={skip} seeds={seeds}"
                assert ("ray_dead" in a) == ("ray_dead" in b) == bool(skip)
                if skip:                                                    # rays the cell grids prove masked are never sampled: no launch writes their index rows
                    assert torch.equal(a["ray_dead"], b["ray_dead"]), what
                    live = a["ray_dead"] == 0
                    assert 0 < int(live.sum()) < N
                    for r_ in (a, b):
                        for k in ("ss_inds", "sort_index"):
                            r_[k] = r_[k][live]
                same_bits(a, b, keys + (["near_m", "far_m"] if guide else []), what)
                assert 0.02 < float(a["mask"].float().mean()) < 0.7 and float(a["weights_sum"].max()) > 0.5


# ------------------------------------------------------------------ 6. repeatability
@pytest.mark.parametrize("precision", ["exact", "fast"])
def test_half_render_repeats_bit_for_bit(env, precision):
    from avatarcraft_amd import nsr_ops
    ro, rd = make_rays(64, 64, dist=1.7, f=50.0)
    ro, rd = t(ro), t(rd)
    first = None
    for _ in range(20):
        o = nsr_ops.render_rays(env["f"], ro, rd, 64, 64, 1.6, env["inv_s"], precision=precision, table_dtype="half")
        cur = {k: o[k].clone() for k in LEAN_KEYS}
        if first is None:
            first = cur
        else:
            same_bits(cur, first, LEAN_KEYS, "repeat")
    assert nsr_ops.handoff_timeouts(DEV) == 0


# ------------------------------------------------------------------ 7. model and drivers
def test_model_and_drivers_route_the_half_table():
    from avatarcraft_amd import nsr_ops, drivers as DR, smpl as SM
    from tests.test_gpu_model import golden_net
    net, p = golden_net()
    net.eval()
    ro, rd = make_rays(16, 16, dist=1.7, f=12.5)
    ro, rd = t(ro), t(rd)
    kw = dict(cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0)

    def model(T0=64, up=64):
        o = net.render(ro[None], rd[None], T0, 1.6, up, **kw)
        return {k: o[k].detach().clone() for k in ("rgb", "depth", "weight_sum", "normal", "z_vals", "weights")}

    def direct(table_dtype):
        o = nsr_ops.render_rays(net._field(), ro, rd, 64, 64, 1.6, net.forward_variance(), extras=True, table_dtype=table_dtype, **kw)
        return dict(rgb=o["image"][None].clone(), depth=o["depth"][None].clone(), weight_sum=o["weights_sum"][:, None].clone(), normal=o["normal_map"].clone(),
                    z_vals=o["z_vals"].clone(), weights=o["weights"].clone())
    keys = ("rgb", "depth", "weight_sum", "normal", "z_vals", "weights")
    with torch.no_grad():
        fp32 = model()
        same_bits(fp32, direct("float"), keys, "default")
        net.render_table_dtype = "half"
        half = model()
        same_bits(half, direct("half"), keys, "half")
        assert not torch.equal(half["rgb"], fp32["rgb"])                        # the rounded table is another field (by ~1e-4)
        assert float((half["rgb"] - fp32["rgb"]).abs().max()) <= 1e-3
        # a parameter step gives a new Field, and with it a new half table
        f_old = net._field()
        with torch.no_grad():
            net.encoder.embeddings[1000:60000] += 0.01                         # (in place: bumps the version counter)
        assert net._field() is not f_old
        moved = model()
        assert not torch.equal(moved["rgb"], half["rgb"])
        fresh = nsr_ops.Field(net.encoder.embeddings.detach().clone(), net._offsets_host(), net.encoder.per_level_scale, net.encoder.base_resolution,
                              *[net._field().t[k] for k in ("W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3")])
        o = nsr_ops.render_rays(fresh, ro, rd, 64, 64, 1.6, net.forward_variance(), extras=True, table_dtype="half", **kw)
        assert torch.equal(o["image"][None], moved["rgb"]) and torch.equal(o["z_vals"], moved["z_vals"])
        with pytest.raises(NotImplementedError, match="fused renderer's window only"):
            net.render(ro[None], rd[None], 128, 1.6, 128, **kw)
        # training mode reads the fp32 table
        net.train()
        same_bits(model(), direct("float"), keys, "train mode")
        net.eval()
    # ... and so does a render that wants gradients
    o = net.render(ro[None], rd[None], 64, 1.6, 64, **kw)
    assert o["rgb"].requires_grad
    with torch.no_grad():
        same_bits({k: o[k].detach() for k in keys}, direct("float"), keys, "under autograd")

    # drivers: the attribute is set around every frame and restored, also when the generator is abandoned
    net.render_table_dtype = "float"
    verts, faces, _ = make_body(n_lat=10, n_lon=12)
    bm = SM.BodyModel.synthetic(seed=2, n_verts=verts.shape[0], faces=faces, v_template=verts)
    cam = np.eye(4, dtype=np.float32); cam[:3, 3] = [0.0, 0.0, 2.2]
    poses = (np.random.RandomState(1).normal(size=(2, 72)) * 0.2).astype(np.float32)
    seen = []
    real = nsr_ops.render_rays

    def spy(*a, **k):
        o = real(*a, **k)
        seen.append((k.get("table_dtype", "float"), o["image"].clone()))
        return o
    anim = lambda **k: DR.render_animation(net, bm, cam, poses=poses, resolution=64, max_frames=2, **k)
    nsr_ops.render_rays = spy
    try:
        frames = list(anim(table_dtype="half"))
    finally:
        nsr_ops.render_rays = real
    assert net.render_table_dtype == "float"
    assert len(frames) == 2 and [s[0] for s in seen] == ["half", "half"]
    for (_, rgb), (_, img) in zip(frames, seen):
        assert torch.equal(rgb.reshape(-1, 3), img.reshape(-1, 3))              # the frame is the half-table launch's image
    net.render_table_dtype = "half"                                             # the same frames with the attribute set by hand, and other than the fp32 frames
    by_hand = list(anim())
    assert net.render_table_dtype == "half"
    net.render_table_dtype = "float"
    fp32_frames = list(anim())
    for a, b, c in zip(frames, by_hand, fp32_frames):
        assert torch.equal(a[1], b[1]) and not torch.equal(a[1], c[1])          # (another field by the rounding: how far is section 5.9's matter, not this test's)
    gen = anim(table_dtype="half")
    next(gen)
    gen.close()
    assert net.render_table_dtype == "float"
    views = list(DR.render_canonical_360(net, n_views=1, render_hw=(16, 16), with_head=False, table_dtype="half"))
    assert net.render_table_dtype == "float" and views[0][2].shape == (16, 16, 3)


# ------------------------------------------------------------------ 8. the raw entries' refusals
def test_raw_entries_refuse_with_the_rule(env):
    from avatarcraft_amd import _lib as L, nsr_ops
    lib = L.lib()
    f = env["f"]
    h = f.half_table()
    N = 16
    ro, rd = make_rays(4, 4)
    ro, rd = t(ro), t(rd)
    lin_z, lin_u = nsr_ops.linspace_tables(64, ro.device)
    bufs = {k: torch.zeros(N * s, device=DEV) for k, s in (("image", 3), ("weights_sum", 1), ("depth", 1), ("normal_map", 3), ("eik", 2))}
    extra = torch.zeros(N * 128 * 16, device=DEV)

    def call(h16=h.data_ptr(), T0=64, up=64, opacity_only=0, **outs):
        o = L.ac_render_out()
        for k, v in bufs.items():
            setattr(o, k, v.data_ptr())
        for k in outs:
            setattr(o, k, extra.data_ptr())
        op = L.ac_render_opts(N, T0, up, 1.6, env["inv_s"], 1.0, 0.005, 0, None, None, None, 0, 0, opacity_only)
        rc = lib.ac_render_rays_h16(C.byref(f.c), h16, C.byref(op), ro.data_ptr(), rd.data_ptr(), None, None, lin_z.data_ptr(), lin_u.data_ptr(), C.byref(o),
                                    L.current_stream(ro.device))
        return rc, lib.ac_last_error().decode()
    assert call()[0] == 0
    for kwargs, rule in ((dict(opacity_only=1), "opacity_only"), (dict(feat7=1), "training extras"), (dict(sdf_out16=1), "training extras"),
                         (dict(pts=1), "training extras"), (dict(T0=128, up=128), "unsupported"), (dict(T0=100, up=64), "unsupported"),
                         (dict(h16=None), "NULL half table")):
        rc, msg = call(**kwargs)
        assert rc != 0 and rule in msg and "render_rays_h16" in msg, (kwargs, rc, msg)
    # the posed entry: the same rules in front of the same sequence
    verts, faces, Ts = make_body(n_lat=10, n_lon=12)
    wm = nsr_ops.WarpMesh(verts, faces, Ts, DEV)
    offs = (C.c_size_t * 6)()
    nbytes = int(lib.ac_render_rays_warped_scratch(N, 128, offs))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    o = L.ac_render_out()
    for k, v in bufs.items():
        setattr(o, k, v.data_ptr())
    for h16, oo, rule in ((None, 0, "NULL half table"), (h.data_ptr(), 1, "opacity_only")):
        op = L.ac_render_opts(N, 64, 64, 1.6, env["inv_s"], 1.0, 0.005, 0, None, None, None, 0, 0, oo)
        rc = lib.ac_render_rays_warped_h16(C.byref(f.c), h16, C.byref(op), ro.data_ptr(), rd.data_ptr(), None, None, lin_z.data_ptr(), lin_u.data_ptr(),
                                           C.byref(wm.c), scratch.data_ptr(), nbytes, C.byref(o), L.current_stream(ro.device))
        assert rc != 0 and rule in lib.ac_last_error().decode() and "render_rays_warped_h16" in lib.ac_last_error().decode()
    torch.cuda.synchronize()
