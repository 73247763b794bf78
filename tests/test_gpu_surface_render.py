"""-m gpu: ac_render_rays_surface (csrc/surface_rays.hip), the first-hit render of the level set, and what stands on it -- nsr_ops.render_rays_surface,
NeRFNetwork.render_surface, drivers.render_canonical_360(surface=True).  Every output is compared BIT FOR BIT with `restate` (tests/surface_cases.py): the
procedure of include/avatarcraft_hip.h in numpy fp32 around the CPU oracle's orc_field_sdf / orc_field_samples.  Measured on the oracle, golden field, bound 1.6,
tol 1e-4, the 588 shared rays: status histogram [453, 0, 128, 1, 6, 0] at the defaults, 10 569 evaluations (18 per ray), max |sdf| over the hits 9.93e-5."""
import numpy as np
import pytest
import torch

from tests import surface_cases as S
from tests.common import load_golden
from tests.gpu_common import assert_bitwise, oracle_field as make_of
from tests.test_gpu_mesh_attrs import oracle_twin
from tests.test_gpu_model import golden_net, DEV

pytestmark = pytest.mark.gpu
F = np.float32
BOUND, EPS = S.BOUND, S.EPS
VARIANTS = {"defaults": {}, "level": dict(level=0.05), "no_guard": dict(guard=0.0)}

_ENV = {}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def env(oracle):
    """the golden field on the device and in the oracle (the same effective weights), the shared rays, the golden net with its own oracle twin, and the
    restatement's results by (variant, max_iters) -- computed once, never modified"""
    if not _ENV:
        from tests.gpu_common import device_field
        p = load_golden("nsr_params.npz")
        gf, table = device_field(p, device=DEV)
        o, d = S.rays()
        net, _ = golden_net()
        bg = np.random.RandomState(3).uniform(0.0, 1.0, o.shape).astype(F)
        _ENV.update(gf=gf, of=make_of(p, table), p=p, o=o, d=d, to=T(o), td=T(d), bg=bg, tbg=T(bg), ref={}, net=net,
                    of_net=oracle_twin(oracle, net, p["offsets"], p["per_level_scale"]))
    return _ENV


def reference(oracle, env, variant="defaults", max_iters=64):
    key = (variant, max_iters)
    if key not in env["ref"]:
        r = S.restate(oracle, env["of"], env["o"], env["d"], max_iters=max_iters, **VARIANTS[variant])
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        env["ref"][key] = r
    return env["ref"][key]


def same(got, want, what, keys=S.OUTPUTS):
    for k in keys:
        assert_bitwise(got[k], want[k], f"{what}: {k}")


def run(env, o=None, d=None, field=None, **kw):
    from avatarcraft_amd import nsr_ops
    return nsr_ops.render_rays_surface(env["gf"] if field is None else field, env["to"] if o is None else o, env["td"] if d is None else d, BOUND, EPS, **kw)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_bit_for_bit_against_the_restatement(oracle, env, variant):
    for mi in (1, 16, 64):
        want = reference(oracle, env, variant, mi)
        hist = np.bincount(want["status"], minlength=6).tolist()
        print(variant, mi, hist, "evaluations", int(want["iters"].astype(np.int64).sum()))
        same(run(env, max_iters=mi, **VARIANTS[variant]), want, f"{variant}, max_iters {mi}, white")
        shaded = np.isin(want["status"], (0, 1, 3))
        with_bg = dict(want, image=np.where(shaded[:, None], want["image"], env["bg"]))
        same(run(env, max_iters=mi, bg=env["tbg"], **VARIANTS[variant]), with_bg, f"{variant}, max_iters {mi}, per-ray bg")
        if variant == "defaults":
            assert hist == S.HIST[mi], (mi, hist)
    d = reference(oracle, env, "defaults", 64)
    assert np.abs(d["sdf"][d["status"] == 0]).max() <= 1.05e-4 and (d["status"] == 0).sum() >= 400
    if variant == "level":
        r = reference(oracle, env, "level", 64)
        hit = r["status"] == 0
        assert hit.sum() >= 400 and np.abs(r["sdf"][hit] - F(0.05)).max() <= 1.05e-4


def test_tile_and_grid_edges(oracle, env):
    full = run(env)
    same(full, reference(oracle, env), "all 588")
    for n in (0, 1, 15, 16, 17, 587):
        part = run(env, env["to"][:n].contiguous(), env["td"][:n].contiguous())
        for k in S.OUTPUTS:
            assert part[k].shape[0] == n and torch.equal(part[k], full[k][:n]), (n, k)
    empty = run(env, env["to"][:0].contiguous(), env["td"][:0].contiguous())
    assert empty["image"].shape == (0, 3) and empty["status"].dtype == torch.uint8 and empty["iters"].dtype == torch.uint8
    big = run(env, env["to"].repeat(150, 1), env["td"].repeat(150, 1))                 # 88 200 rays: every workgroup takes several tiles
    for k in S.OUTPUTS:
        assert big[k].shape[0] == 88200 and torch.equal(big[k].reshape(150, 588, -1), full[k].reshape(1, 588, -1).expand(150, -1, -1)), k
    # a tile of 16 rays that all miss the cube (no shaded ray: neither stencil nor colour) next to shaded tiles
    miss = int(np.flatnonzero(reference(oracle, env)["iters"] == 0)[0])                # far <= near: no evaluation at all
    o = torch.cat([env["to"][miss:miss + 1].repeat(16, 1), env["to"]]); d = torch.cat([env["td"][miss:miss + 1].repeat(16, 1), env["td"]])
    bg = torch.cat([env["tbg"][:16], env["tbg"]])
    r = run(env, o, d, bg=bg)
    assert bool((r["status"][:16] == 2).all()) and bool((r["iters"][:16] == 0).all()) and torch.equal(r["image"][:16], bg[:16])
    assert all(bool((r[k][:16] == 0).all()) for k in ("weights_sum", "depth", "position", "normal_map", "sdf"))
    withbg = run(env, bg=env["tbg"])
    for k in S.OUTPUTS:
        assert torch.equal(r[k][16:], withbg[k]), k
    again = run(env)
    assert all(torch.equal(again[k], full[k]) for k in S.OUTPUTS)


def test_geometry_only_mode(env):
    net = env["net"]
    with torch.no_grad():
        full = run(env, field=net._field())
        for field in (net._field(), net._field_sdf_only()):                             # the second has placeholder colour matrices
            geo = run(env, field=field, want_rgb=False)
            assert geo["image"] is None and all(torch.equal(geo[k], full[k]) for k in S.OUTPUTS if k != "image")
    assert int((full["status"] == 0).sum()) >= 400


def test_view_directions(oracle, env):
    from tests.test_gpu_viewdirs import viewdirs_net
    g = load_golden("viewdirs.npz")
    net = viewdirs_net(g)
    of = oracle_twin(oracle, net, g["offsets"], g["per_level_scale"])
    assert of.has_viewdirs and net._field().has_viewdirs
    with torch.no_grad():
        got = run(env, field=net._field())
    want = S.restate(oracle, of, env["o"], env["d"])
    same(got, want, "dirs = rays_d")
    shaded = np.isin(want["status"], (0, 1, 3))
    assert shaded.sum() >= 100
    # the same points seen along other directions have other colours: the ray's own direction is what reaches the colour network
    other = S.restate(oracle, of, env["o"], env["d"], dirs=np.roll(env["d"], 7, axis=0))
    assert np.array_equal(other["position"], want["position"]) and np.array_equal(other["normal_map"], want["normal_map"])
    differ = np.any(other["image"] != want["image"], axis=1)
    assert differ[shaded].mean() > 0.9, differ[shaded].mean()
    # two rays through one hit point: the second aims at the first's hit from a camera 0.4 to the side
    i = int(np.flatnonzero(want["status"] == 0)[len(np.flatnonzero(want["status"] == 0)) // 2])
    P = want["position"][i].astype(np.float64)
    o2 = env["o"][i].astype(np.float64) + np.array([0.4, 0.0, 0.0])
    d2 = (P - o2) / np.linalg.norm(P - o2)
    with torch.no_grad():
        two = run(env, T(np.stack([env["o"][i], o2.astype(F)])), T(np.stack([env["d"][i], d2.astype(F)])), field=net._field())
    pos, rgb, st = two["position"].cpu().numpy(), two["image"].cpu().numpy(), two["status"].cpu().numpy()
    print("two rays: status", st.tolist(), "distance of the hit points", float(np.abs(pos[0] - pos[1]).max()), "rgb", rgb.tolist())
    assert st.tolist() == [0, 0] and np.array_equal(pos[0], want["position"][i]) and np.abs(pos[0] - pos[1]).max() <= 2e-3
    assert not np.array_equal(rgb[0], rgb[1])


def test_nan_field_gives_status_5(oracle, env):
    from avatarcraft_amd import nsr_ops
    f, p = env["gf"], env["p"]
    nan_table = torch.full_like(f.t["table"], float("nan"))
    nf = nsr_ops.Field(nan_table, [int(o) for o in p["offsets"]], float(p["per_level_scale"]), 16, f.t["W1"], f.t["b1"], f.t["W2"], f.t["b2"],
                       f.t["Wc1"], f.t["Wc2"], f.t["Wc3"])
    r = run(env, field=nf, bg=env["tbg"])
    near, far = oracle._near_far_cube(env["o"], env["d"], BOUND)
    inside = T(far > near)
    assert 0 < int(inside.sum()) < 588
    assert bool((r["status"][inside] == 5).all()) and bool((r["iters"][inside] == 1).all())
    assert bool((r["status"][~inside] == 2).all()) and bool((r["iters"][~inside] == 0).all())
    assert torch.equal(r["image"], env["tbg"])
    assert all(bool((r[k] == 0).all()) for k in ("weights_sum", "depth", "position", "normal_map", "sdf"))


def test_model_and_driver(oracle, env):
    from avatarcraft_amd import nsr_ops, drivers
    net = env["net"]
    o, d = S.pinhole((0.3, 0.4, 2.6), n=16, fov=0.5)
    to, td = T(o), T(d)
    with torch.no_grad():
        m = net.render_surface(to[None], td[None], BOUND)
        k = nsr_ops.render_rays_surface(net._field(), to, td, BOUND, nsr_ops.FD_STEP)
        batched = net.render_surface(to[None], td[None], BOUND, max_ray_batch=100)
        black = net.render_surface(to[None], td[None], BOUND, bg_color=0.0, max_iters=16, want_rgb=True)
    assert set(m) == {"rgb", "depth", "weight_sum", "normal", "position", "sdf", "status", "iters"}
    assert m["rgb"].shape == (1, 256, 3) and m["depth"].shape == (1, 256) and m["weight_sum"].shape == (256, 1) and m["normal"].shape == (256, 3)
    for a, b in (("rgb", "image"), ("depth", "depth"), ("weight_sum", "weights_sum"), ("normal", "normal_map"), ("position", "position"), ("sdf", "sdf"),
                 ("status", "status"), ("iters", "iters")):
        assert torch.equal(m[a].reshape(k[b].shape), k[b]), a
        assert torch.equal(batched[a], m[a]), a
    hit = m["weight_sum"][:, 0] == 1
    assert 0 < int(hit.sum()) < 256 and bool((black["rgb"][0][black["weight_sum"][:, 0] == 0] == 0).all()) and int(black["iters"].max()) <= 16
    with torch.enable_grad():
        assert any(p.requires_grad for p in net.parameters())
        with pytest.raises(RuntimeError, match="no_grad"):
            net.render_surface(to[None], td[None], BOUND)
    with pytest.raises(RuntimeError, match="max_iters"):
        with torch.no_grad():
            net.render_surface(to[None], td[None], BOUND, max_iters=0)
    views = list(drivers.render_canonical_360(net, n_views=2, render_hw=(16, 16), with_head=False, surface=True))
    assert [(v[0], v[1]) for v in views] == [("body", 0), ("body", 1)]
    from avatarcraft_amd.render_utils import default_360_path, pose2cap, cap2rays
    poses = default_360_path(np.zeros(3), np.array([0.0, 1.0, 0.0]), drivers.CANONICAL_CAMERA_DIST_VAL, 2)[0]
    for (_, i, rgb, depth), pose in zip(views, poses):
        assert rgb.shape == (16, 16, 3) and depth.shape == (16, 16) and bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all())
        assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0
        ro, rd = cap2rays(pose2cap([16, 16], pose), device=DEV)
        with torch.no_grad():
            r = net.render_surface(ro.reshape(1, -1, 3), rd.reshape(1, -1, 3), BOUND)
        assert torch.equal(r["rgb"].reshape(16, 16, 3), rgb) and torch.equal(r["depth"].reshape(16, 16), depth)
        near, far = (T(a) for a in oracle._near_far_cube(ro.reshape(-1, 3).cpu().numpy(), rd.reshape(-1, 3).cpu().numpy(), BOUND))
        w, dep = r["weight_sum"][:, 0] == 1, depth.reshape(-1)
        assert int(w.sum()) > 0 and bool(((dep[w] >= near[w]) & (dep[w] <= far[w])).all()) and bool((dep[~w] == 0).all())


def test_same_level_set_as_the_export(oracle, env):
    """rays from a camera outside the cube towards every vertex of extract_colored_mesh(1.6, 48): where the ray is a hit it ends ON the level set, at or in front
    of the vertex.  On the CPU oracle (golden field, the oracle's own marching cubes and three Newton steps) 791 of the 812 rays are status 0, the other 21
    run out of iterations without a bracket (status 4); max t - |vertex - origin| over the hits 5.3e-4."""
    net = env["net"]
    v = net.extract_colored_mesh(BOUND, 48)["vertices"]
    assert v.shape == (812, 3)
    o = np.broadcast_to(np.array([0.3, 0.4, 2.6], F), v.shape).copy()
    d64 = v - o.astype(np.float64)
    dist = np.linalg.norm(d64, axis=1)
    d = (d64 / dist[:, None]).astype(F)
    with torch.no_grad():
        got = run(env, T(o), T(d), field=net._field())
    want = S.restate(oracle, env["of_net"], o, d)
    same(got, want, "rays at the mesh vertices")
    st = got["status"].cpu().numpy()
    hit = st == 0
    print("status histogram", np.bincount(st, minlength=6).tolist(), "max t - dist over the hits", float((want["depth"][hit] - dist[hit]).max()))
    assert hit.sum() >= 791
    assert np.abs(want["sdf"][hit]).max() <= 1.05e-4 and float(got["sdf"][T(hit)].abs().max()) <= 1.05e-4
    assert (got["depth"].cpu().numpy()[hit] <= dist[hit] + 1e-3).all()
