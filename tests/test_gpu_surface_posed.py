"""-m gpu: ac_render_rays_surface_warped (csrc/surface_rays.hip), the first-hit render of the POSED level set, and what stands on it --
nsr_ops.render_rays_surface_warped, NeRFNetwork.render_surface_posed, drivers.render_animation(surface=True).  Every output is compared BIT FOR BIT with
`restate_posed` (tests/surface_posed_cases.py): the procedure of include/avatarcraft_hip.h in numpy around the CPU oracle's orc_warp_samples / orc_field_sdf /
orc_field_samples.  What the procedure achieves on the shared case is recorded on the CPU tier (tests/test_surface_posed_host.py)."""
import numpy as np
import pytest
import torch

from tests import mesh_pose_cases as MC
from tests import surface_cases as S
from tests import surface_posed_cases as P
from tests.common import load_golden
from tests.gpu_common import assert_bitwise, oracle_field as make_of
from tests.test_gpu_mesh_attrs import oracle_twin
from tests.test_gpu_model import golden_net, DEV

pytestmark = pytest.mark.gpu
F = np.float32
BOUND, EPS = P.BOUND, P.EPS
VARIANTS = {"defaults": {}, "level": dict(level=0.05), "no_guard": dict(guard=0.0), "no_w_tol": dict(w_tol=0.0)}

_ENV = {}


def T(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                  # (a copy: the shared case is read-only)


@pytest.fixture(scope="module")
def env(oracle):
    """the golden field on the device and in the oracle, the shared rays and body (with and without the culling structure), and the restatement's results by
    (variant, max_iters) -- computed once, never modified"""
    if not _ENV:
        from avatarcraft_amd import nsr_ops
        from tests.gpu_common import device_field
        p = load_golden("nsr_params.npz")
        gf, table = device_field(p, device=DEV)
        o, d = P.rays()
        v, f, Ts = P.body()
        bg = np.random.RandomState(3).uniform(0.0, 1.0, o.shape).astype(F)
        wm = {a: nsr_ops.WarpMesh(v.copy(), f.copy(), Ts.copy(), DEV, threshold=P.THRESHOLD, accel=a) for a in (True, False)}
        assert wm[True].accel is not None and wm[False].accel is None
        _ENV.update(gf=gf, of=make_of(p, table), table=table, p=p, o=o, d=d, to=T(o), td=T(d), bg=bg, tbg=T(bg), body=(v, f, Ts), wm=wm, ref={})
    return _ENV


def reference(oracle, env, variant="defaults", max_iters=64):
    key = (variant, max_iters)
    if key not in env["ref"]:
        r = P.restate_posed(oracle, env["of"], env["o"], env["d"], *env["body"], max_iters=max_iters, **VARIANTS[variant])
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        env["ref"][key] = r
    return env["ref"][key]


def same(got, want, what, keys=P.OUTPUTS):
    for k in keys:
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def run(env, o=None, d=None, field=None, accel=True, warp=None, **kw):
    from avatarcraft_amd import nsr_ops
    return nsr_ops.render_rays_surface_warped(env["gf"] if field is None else field, env["to"] if o is None else o, env["td"] if d is None else d, BOUND,
                                              env["wm"][accel] if warp is None else warp, EPS, **kw)


@pytest.mark.parametrize("max_iters", [64, 16, 1])
def test_bit_for_bit_against_the_restatement(oracle, env, max_iters):
    want = reference(oracle, env, "defaults", max_iters)
    hist = np.bincount(want["status"], minlength=7).tolist()
    print(max_iters, hist, "searches", want["trace"]["searches"], "sdf evaluations", want["trace"]["sdf_evals"])
    assert hist == P.HIST_ALL[max_iters]
    shaded = np.isin(want["status"], P.SHADED)
    with_bg = dict(want, image=np.where(shaded[:, None], want["image"], env["bg"]))
    for accel in (True, False):                                                   # the culled and the exhaustive search: identical bits
        same(run(env, accel=accel, max_iters=max_iters), want, f"max_iters {max_iters}, accel {accel}, white")
        same(run(env, accel=accel, max_iters=max_iters, bg=env["tbg"]), with_bg, f"max_iters {max_iters}, accel {accel}, per-ray bg")


@pytest.mark.parametrize("variant", ["level", "no_guard", "no_w_tol"])
def test_options_bit_for_bit(oracle, env, variant):
    want = reference(oracle, env, variant, 64)
    print(variant, np.bincount(want["status"], minlength=7).tolist())
    same(run(env, **VARIANTS[variant]), want, variant)
    if variant == "level":
        hit = want["status"] == 0
        assert hit.sum() >= 20 and np.abs(want["sdf"][hit] - F(0.05)).max() <= 1.05e-4
    if variant == "no_w_tol":                                                     # a bracket never closes to width 0 on this case: cuts run out of iterations
        assert (want["status"] != 6).all() and (want["status"] == 1).sum() >= 20


def test_tile_and_grid_edges(oracle, env):
    full = run(env, bg=env["tbg"])
    for n in (0, 1, 15, 16, 17, 415):
        part = run(env, env["to"][:n].contiguous(), env["td"][:n].contiguous(), bg=env["tbg"][:n].contiguous())
        for k in P.OUTPUTS:
            assert part[k].shape[0] == n and torch.equal(part[k], full[k][:n]), (n, k)
    empty = run(env, env["to"][:0].contiguous(), env["td"][:0].contiguous())
    assert empty["image"].shape == (0, 3) and empty["status"].dtype == torch.uint8 and empty["face_id"].dtype == torch.int32
    # a tile of 16 rays that all miss the cube (no search, no evaluation, no shading) next to shaded tiles
    miss = int(np.flatnonzero(reference(oracle, env)["iters"] == 0)[0])
    o = torch.cat([env["to"][miss:miss + 1].repeat(16, 1), env["to"]]); d = torch.cat([env["td"][miss:miss + 1].repeat(16, 1), env["td"]])
    bg = torch.cat([env["tbg"][:16], env["tbg"]])
    r = run(env, o, d, bg=bg)
    assert bool((r["status"][:16] == 2).all()) and bool((r["iters"][:16] == 0).all()) and torch.equal(r["image"][:16], bg[:16])
    assert all(bool((r[k][:16] == 0).all()) for k in ("weights_sum", "depth", "position", "normal_map", "sdf", "canonical", "normal_can"))
    assert bool((r["face_id"][:16] == -1).all())
    for k in P.OUTPUTS:
        assert torch.equal(r[k][16:], full[k]), k
    big = run(env, env["to"].repeat(40, 1), env["td"].repeat(40, 1), bg=env["tbg"].repeat(40, 1))      # 16 600 rays: several tiles per wave
    for k in P.OUTPUTS:
        assert torch.equal(big[k].reshape(40, 415, -1), full[k].reshape(1, 415, -1).expand(40, -1, -1)), k


def test_geometry_only_and_view_directions(oracle, env):
    from tests.test_gpu_viewdirs import viewdirs_net
    net, _ = golden_net()
    with torch.no_grad():
        full = run(env, field=net._field())
        for field in (net._field(), net._field_sdf_only()):                       # the second has placeholder colour matrices
            geo = run(env, field=field, want_rgb=False)
            assert geo["image"] is None and all(torch.equal(geo[k], full[k]) for k in P.OUTPUTS if k != "image")
    assert int((full["weights_sum"] == 1).sum()) >= 60
    g = load_golden("viewdirs.npz")
    vnet = viewdirs_net(g)
    of = oracle_twin(oracle, vnet, g["offsets"], g["per_level_scale"])
    assert of.has_viewdirs and vnet._field().has_viewdirs
    with torch.no_grad():
        got = run(env, field=vnet._field())
    want = P.restate_posed(oracle, of, env["o"], env["d"], *env["body"])
    same(got, want, "dirs = rays_d")
    shaded = np.isin(want["status"], P.SHADED)
    other = P.restate_posed(oracle, of, env["o"], env["d"], *env["body"], dirs=np.roll(env["d"], 7, axis=0))
    assert np.array_equal(other["position"], want["position"]) and shaded.sum() >= 20
    assert np.any(other["image"] != want["image"], axis=1)[shaded].mean() > 0.9  # the ray's own direction is what reaches the colour network


def test_nan_field_gives_status_5(oracle, env):
    from avatarcraft_amd import nsr_ops
    f, p = env["gf"], env["p"]
    nan_table = torch.full_like(f.t["table"], float("nan"))
    nf = nsr_ops.Field(nan_table, [int(o) for o in p["offsets"]], float(p["per_level_scale"]), 16, f.t["W1"], f.t["b1"], f.t["W2"], f.t["b2"],
                       f.t["Wc1"], f.t["Wc2"], f.t["Wc3"])
    onf = oracle.Field(np.full_like(env["table"], np.nan), p["offsets"], p["W1"], p["b1"], p["W2"], p["b2"], p["Wc1"], p["Wc2"], p["Wc3"], float(p["per_level_scale"]))
    want = P.restate_posed(oracle, onf, env["o"], env["d"], *env["body"], bg=env["bg"])
    r = run(env, field=nf, bg=env["tbg"])
    same(r, want, "NaN table")
    hist = np.bincount(want["status"], minlength=7).tolist()
    print(hist)
    assert hist[5] >= 60 and hist[2] + hist[5] == 415                             # every ray that reaches the mask stops at its first unmasked point
    assert torch.equal(r["image"], env["tbg"]) and bool((r["face_id"] == -1).all())
    assert all(bool((r[k] == 0).all()) for k in ("weights_sum", "depth", "position", "normal_map", "sdf", "canonical", "normal_can"))


def test_identity_warp_is_the_canonical_render(oracle, env):
    """identity transforms and a threshold under which every point of the cube is unmasked: can = p, the traced function is the canonical SDF everywhere, and with
    w_tol = 0 the procedure is ac_render_rays_surface's -- status, iters, depth, position, sdf and image equal that entry's bit for bit (no ray of this set stops
    with status 1, where the two report different ends of the bracket).  The posed normal is ac_mesh_pose's rule on the identity: the canonical normal
    g / (1e-5 + |g|) divided by its own length in fp64 -- equal to normal_can up to that renormalisation, which is restated here."""
    from avatarcraft_amd import nsr_ops
    v, f, _ = env["body"]
    I = np.tile(np.eye(4)[None], (len(v), 1, 1))
    o, d = S.rays()
    to, td = T(o), T(d)
    can = nsr_ops.render_rays_surface(env["gf"], to, td, BOUND, EPS)
    assert int((can["status"] == 1).sum()) == 0 and int((can["status"] == 0).sum()) >= 400
    for accel in (True, False):
        wm = nsr_ops.WarpMesh(v.copy(), f.copy(), I, DEV, threshold=100.0, accel=accel)
        got = run(env, to, td, warp=wm, w_tol=0.0)
        for k in ("status", "iters", "depth", "position", "sdf", "image", "weights_sum"):
            assert torch.equal(got[k], can[k]), (accel, k)
        assert torch.equal(got["canonical"], got["position"]) and torch.equal(got["normal_can"], can["normal_map"])
        nc = got["normal_can"].cpu().numpy()
        sh = got["weights_sum"].cpu().numpy() == 1
        want = np.zeros_like(nc)
        want[sh] = MC.warp_normal(I[:int(sh.sum())], nc[sh])
        assert_bitwise(got["normal_map"], want, "posed normal on the identity")
        assert float((got["normal_map"] - got["normal_can"]).abs().max()) <= 1e-4


# largest t - |vertex - origin| over the status-0 rays, measured on the CPU restatement (golden net, 48^3 mesh, frame 5): 4.70e-4; the margin is twice that
POSED_VERTEX_MARGIN = 9.4e-4


def test_same_posed_set_as_pose_mesh(oracle, env):
    """rays from a camera outside the body towards the vertices pose_mesh returns with status 0 for frame 5 of the smooth body sequence (canonical mesh:
    extract_colored_mesh(1.6, 48)): where the ray is a hit (status 0) it ends ON the posed level set, at or in front of the vertex.  On the CPU restatement: 415 of the 812 vertices come back with status 0; of their rays 251 are hits,
    153 end on the mask boundary (status 6: the golden sphere is wider than the capsule's mask) and 11 run out of iterations without a bracket."""
    from avatarcraft_amd import nsr_ops
    vs, faces, Ts = MC.smooth_body_sequence()
    net, _ = golden_net()
    net.eval()
    mesh = net.extract_colored_mesh(BOUND, 48, return_torch=True)
    guide = dict(faces=faces.copy())
    posed = net.pose_mesh(mesh, guide, vs[5].copy(), Ts[5].copy())
    ok = (posed["status"] == 0).cpu().numpy()
    v = posed["vertices"].cpu().numpy()[ok]
    assert len(v) >= 400
    o = np.broadcast_to(np.array([0.3, 0.4, 2.6], F), v.shape).copy()
    d64 = v - o.astype(np.float64)
    dist = np.linalg.norm(d64, axis=1)
    d = (d64 / dist[:, None]).astype(F)
    wm = nsr_ops.WarpMesh(vs[5].copy(), faces.copy(), Ts[5].copy(), DEV, threshold=MC.THRESHOLD)
    with torch.no_grad():
        got = run(env, T(o), T(d), field=net._field(), warp=wm)
    p = load_golden("nsr_params.npz")
    want = P.restate_posed(oracle, oracle_twin(oracle, net, p["offsets"], p["per_level_scale"]), o, d, vs[5], faces, Ts[5], threshold=MC.THRESHOLD)
    same(got, want, "rays at the posed vertices")
    st = want["status"]
    hit = st == 0
    excess = float((want["depth"][hit] - dist[hit]).max())
    print("vertices", len(v), "status histogram", np.bincount(st, minlength=7).tolist(), "max t - dist over the hits", excess)
    assert hit.sum() >= 251 and np.abs(want["sdf"][hit]).max() <= 1.05e-4
    assert (got["depth"].cpu().numpy()[hit] <= dist[hit] + POSED_VERTEX_MARGIN).all()


def test_stopped_rays_cost_no_search(oracle, env):
    from avatarcraft_amd import nsr_ops
    v, f, Ts = env["body"]
    wm = nsr_ops.WarpMesh(v.copy(), f.copy(), Ts.copy(), DEV, threshold=P.THRESHOLD)
    count = lambda: wm.work_counters()["exact_tests"]
    c0 = count()
    r = run(env, warp=wm, max_iters=64)
    c1 = count()
    k = int(r["iters"].max())
    assert 16 < k < 64
    r2 = run(env, warp=wm, max_iters=k)
    c2 = count()
    assert all(torch.equal(r[x], r2[x]) for x in P.OUTPUTS)
    print("exact tests per call", c1 - c0, "largest iters", k)
    assert c1 - c0 == c2 - c1 and c1 > c0                                         # the 64 - k trips after the last ray stopped searched nothing
    miss = int(np.flatnonzero(reference(oracle, env)["iters"] == 0)[0])
    run(env, env["to"][miss:miss + 1].repeat(64, 1), env["td"][miss:miss + 1].repeat(64, 1), warp=wm)
    assert count() == c2                                                          # 64 rays that miss the cube: not one exact test


def test_model_and_driver(env):
    from avatarcraft_amd import nsr_ops, drivers as DR, smpl as SM
    from avatarcraft_amd.render_utils import render_instantnsr_naive
    from tests.common import make_body
    net, _ = golden_net()
    net.eval()
    v, f, Ts = env["body"]
    to, td = env["to"][:400], env["td"][:400]
    with torch.no_grad():
        m = net.render_surface_posed(to[None], td[None], BOUND, v.copy(), f.copy(), Ts.copy())
        k = nsr_ops.render_rays_surface_warped(net._field(), to.contiguous(), td.contiguous(), BOUND, env["wm"][True])
        batched = net.render_surface_posed(to[None], td[None], BOUND, env["wm"][True], None, None, max_ray_batch=100)
        black = net.render_surface_posed(to[None], td[None], BOUND, env["wm"][True], None, None, bg_color=0.0, max_iters=16)
    assert set(m) == {"rgb", "depth", "weight_sum", "normal", "position", "sdf", "status", "iters", "canonical", "normal_can", "face_id"}
    assert m["rgb"].shape == (1, 400, 3) and m["depth"].shape == (1, 400) and m["weight_sum"].shape == (400, 1) and m["normal"].shape == (400, 3)
    assert m["canonical"].shape == (1, 400, 3) and m["normal_can"].shape == (400, 3) and m["face_id"].shape == (1, 400)
    for a, b in (("rgb", "image"), ("depth", "depth"), ("weight_sum", "weights_sum"), ("normal", "normal_map"), ("position", "position"), ("sdf", "sdf"),
                 ("status", "status"), ("iters", "iters"), ("canonical", "canonical"), ("normal_can", "normal_can"), ("face_id", "face_id")):
        assert torch.equal(m[a].reshape(k[b].shape), k[b]), a
        assert torch.equal(batched[a], m[a]), a
    hit = m["weight_sum"][:, 0] == 1
    assert 60 <= int(hit.sum()) <= 90 and bool((black["rgb"][0][black["weight_sum"][:, 0] == 0] == 0).all()) and int(black["iters"].max()) <= 16
    with torch.enable_grad():
        assert any(p.requires_grad for p in net.parameters())
        with pytest.raises(RuntimeError, match="no_grad"):
            net.render_surface_posed(to[None], td[None], BOUND, env["wm"][True], None, None)
    with pytest.raises(RuntimeError, match="w_tol"):
        with torch.no_grad():
            net.render_surface_posed(to[None], td[None], BOUND, env["wm"][True], None, None, w_tol=-1.0)
    # the driver: two 32 x 32 frames == the method on the frame's arrays; the default path still yields (index, rgb) of the volumetric posed render
    bv, bf, _ = make_body(n_lat=10, n_lon=12)
    bm = SM.BodyModel.synthetic(seed=2, n_verts=bv.shape[0], faces=bf, v_template=bv)
    cam = np.eye(4, dtype=np.float32); cam[:3, 3] = [0.0, 0.0, 2.2]
    poses = (np.random.RandomState(1).normal(size=(2, 72)) * 0.2).astype(np.float32)
    frames = list(DR.render_animation(net, bm, cam, poses=poses, resolution=32, max_frames=2, surface=True))
    wv, wT, n = SM.calc_local_trans(bm, render_type="animate", poses=poses, max_frames=2)
    ro, rd = DR.gen_rays_pose(cam, 16, device=DEV)
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    assert n == 2 and [fr[0] for fr in frames] == [0, 1] and all(len(fr) == 3 for fr in frames)
    shaded = 0
    for i, rgb, depth in frames:
        with torch.no_grad():
            r = net.render_surface_posed(ro[None], rd[None], DR.NSR_BOUND, wv[i], np.asarray(bm.faces), wT[i])
        assert rgb.shape == (32, 32, 3) and depth.shape == (32, 32)
        assert torch.equal(r["rgb"].reshape(32, 32, 3), rgb) and torch.equal(r["depth"].reshape(32, 32), depth)
        shaded += int((r["weight_sum"] == 1).sum())
    assert shaded > 0
    default = list(DR.render_animation(net, bm, cam, poses=poses, resolution=32, max_frames=2))
    assert [len(fr) for fr in default] == [2, 2]
    for i, rgb in default:
        direct, _, _ = render_instantnsr_naive(net, ro, rd, 32 * 32, requires_grad=False, return_torch=True, perturb=False, return_raw=True, render_can=False,
                                               verts=wv[i], faces=np.asarray(bm.faces), Ts=wT[i], num_steps=32, upsample_steps=32, bound=DR.NSR_BOUND)
        assert torch.equal(direct.reshape(32, 32, 3), rgb)
