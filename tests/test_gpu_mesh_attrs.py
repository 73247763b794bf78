"""-m gpu: ac_mesh_vertex_attrs (csrc/mesh_shade.hip) and the coloured export around it -- NeRFNetwork.extract_colored_mesh, nsr_ops.mesh_vertex_attrs.
The kernel projects marching-cubes vertices onto the level set by Newton steps along the finite-difference gradient and evaluates normal and colour there;
every output is compared BIT FOR BIT with `restate`, the loop of include/avatarcraft_hip.h written in numpy fp32 around the CPU oracle's
orc_field_samples.  Measured on the oracle, golden field, bound 1.6, eps 0.005: max |sdf| 4.7e-3 at the 48^3 marching-cubes vertices, 4.9e-5 after 3 steps."""
import numpy as np
import pytest
import torch

from tests.common import load_golden
from tests.gpu_common import assert_bitwise, oracle_field as make_of
from tests.test_gpu_model import golden_net, DEV

pytestmark = pytest.mark.gpu
BOUND, EPS, TOL = 1.6, 0.005, 1e-5
F = np.float32


def restate(O, of, verts, steps, max_move, tol=TOL, target=0.0, dirs=None, bound=BOUND, eps=EPS):
    """the per-vertex arithmetic of ac_mesh_vertex_attrs in numpy fp32 (every operation rounds once, in the kernel's order) around the oracle's stencil"""
    p = np.clip(np.asarray(verts, np.float64).astype(F), F(-bound), F(bound)); p0 = p.copy()
    V = len(p)
    st = np.ones(V, np.uint8); moving = np.ones(V, bool)
    zero, one = np.zeros((V, 3), F), np.ones(V, F)
    ev = lambda x, d: O.field_samples(of, x, d, one, bound, eps, 64.0)
    target, tol, max_move = F(target), F(tol), F(max_move)
    for _ in range(steps):
        if not moving.any():
            break
        fs = ev(p, zero)
        s, g = fs["sdf"], fs["gradient"]
        r = s - target
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        conv = np.abs(r) <= tol
        degen = ~conv & ~(gg > F(1e-12))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = r / gg
        q = np.clip(p - t[:, None] * g, F(-bound), F(bound))
        far = ~conv & ~degen & (np.abs(q - p0).max(1) > max_move)
        st[moving & conv] = 0; st[moving & degen] = 2; st[moving & far] = 3
        moving &= ~(conv | degen | far)
        p = np.where(moving[:, None], q, p)
    assert p.dtype == F
    fs = ev(p, zero)
    if dirs is None:
        dirs = -fs["normal"]
    fs = ev(p, np.ascontiguousarray(dirs, F))
    return dict(positions=p, normals=fs["normal"], rgb=fs["rgb"], sdf=fs["sdf"], status=st)


def same(got, want, what, rgb=True):
    for k in ("positions", "normals", "sdf") + (("rgb",) if rgb else ()):
        assert_bitwise(got[k], want[k], f"{what}: {k}")
    assert np.array_equal(got["status"].cpu().numpy(), want["status"]), what


_ENV = {}


def device_mesh(field, res, iso=0.0):
    """the device pipeline extract_geometry runs (ac_field_sdf_grid + ac_marching_cubes_*) on a given field"""
    from avatarcraft_amd import nsr_ops
    ax = torch.linspace(-BOUND, BOUND, res).to(DEV)
    u = nsr_ops.field_sdf_grid(field, ax, ax, ax, BOUND, negate=True)
    return nsr_ops.marching_cubes(u, iso, den=res - 1.0, span=[float(F(BOUND) - F(-BOUND))] * 3, lo=[float(F(-BOUND))] * 3)


def oracle_twin(oracle, net, offsets, per_level_scale):
    """the oracle's field from THIS net's effective matrices (the device's weight norm): the goldens' effective weights were formed by torch's CPU weight
    norm and differ from them in the last ulp, and the comparisons here are bitwise (as in tests/test_gpu_run_cuda.py)"""
    W = [w.detach().cpu().numpy() for w in net._effective_weights()]
    c = lambda t: t.detach().cpu().numpy()
    return oracle.Field(c(net.encoder.embeddings), offsets, W[0], c(net.sdf_net[0].bias), W[1], c(net.sdf_net[1].bias), W[2], W[3], W[4], float(per_level_scale))


@pytest.fixture(scope="module")
def env(oracle):
    """the golden field on the device and in the oracle (the same effective weights), its marching-cubes vertices from the device pipeline at 24^3 and 48^3,
    and the golden net with its own oracle twin -- built once, never modified"""
    if not _ENV:
        from tests.gpu_common import device_field
        p = load_golden("nsr_params.npz")
        gf, table = device_field(p, device=DEV)
        meshes = {res: device_mesh(gf, res) for res in (24, 48)}
        assert meshes[24][0].shape[0] == 184 and meshes[48][0].shape[0] == 812
        net, _ = golden_net()
        _ENV.update(gf=gf, of=make_of(p, table), p=p, meshes=meshes, ref={}, net=net, of_net=oracle_twin(oracle, net, p["offsets"], p["per_level_scale"]))
    return _ENV


def cell(res):
    return 2.0 * BOUND / (res - 1.0)


def reference(oracle, env, res, steps):
    key = (res, steps)
    if key not in env["ref"]:
        env["ref"][key] = restate(oracle, env["of"], env["meshes"][res][0].cpu().numpy(), steps, cell(res))
    return env["ref"][key]


@pytest.mark.parametrize("res", [24, 48])
def test_bit_for_bit_against_the_oracle(oracle, env, res):
    from avatarcraft_amd import nsr_ops
    f, v = env["gf"], env["meshes"][res][0]
    for steps in (0, 1, 3):
        got = nsr_ops.mesh_vertex_attrs(f, v, BOUND, EPS, refine_steps=steps, tol=TOL, max_move=cell(res))
        want = reference(oracle, env, res, steps)
        same(got, want, f"{res}^3, {steps} steps")
        # the default model's colour is forward_color on the final point, its normal and the SDF network's features there
        p = want["positions"]
        assert_bitwise(got["rgb"], env["of"].color(p, want["normals"], env["of"].sdf(p, BOUND)), "rgb == Field.color")
    hist = np.bincount(reference(oracle, env, res, 3)["status"], minlength=4).tolist()
    assert hist == {48: [678, 134, 0, 0], 24: [124, 60, 0, 0]}[res], hist            # (a silently frozen vertex would show here)
    assert np.abs(reference(oracle, env, res, 0)["sdf"]).max() > 4e-3 and np.abs(reference(oracle, env, res, 3)["sdf"]).max() < 1e-4


def test_tile_and_grid_edges(env):
    from avatarcraft_amd import nsr_ops
    f, v = env["gf"], env["meshes"][48][0]
    run = lambda x: nsr_ops.mesh_vertex_attrs(f, x, BOUND, EPS, refine_steps=3, tol=TOL, max_move=cell(48))
    full = run(v)
    for n in (1, 17, 811):
        part = run(v[:n].contiguous())
        for k, t in part.items():
            assert t.shape[0] == n and torch.equal(t, full[k][:n]), (n, k)
    empty = run(v[:0].contiguous())
    assert all(t.shape[0] == 0 for t in empty.values()) and empty["positions"].shape == (0, 3) and empty["status"].dtype == torch.uint8
    big = run(v.repeat(100, 1))                                                      # 81 200 vertices: every workgroup takes several tiles
    for k, t in big.items():
        assert t.shape[0] == 81200 and torch.equal(t.reshape(100, 812, -1), full[k].reshape(1, 812, -1).expand(100, -1, -1)), k
    again = run(v)
    assert all(torch.equal(again[k], full[k]) for k in full)


def test_stop_conditions(oracle, env):
    from avatarcraft_amd import nsr_ops
    net, of = env["net"], env["of"]
    f, v = env["gf"], env["meshes"][48][0]
    h = cell(48)
    # (a) vertices two cells off the surface: a full Newton step would leave the one-cell box
    shifted = v.clone(); shifted[:, 0] += 2.0 * h
    got = nsr_ops.mesh_vertex_attrs(f, shifted, BOUND, EPS, refine_steps=3, tol=TOL, max_move=h)
    want = restate(oracle, of, shifted.cpu().numpy(), 3, h)
    same(got, want, "shifted")
    st = got["status"].cpu().numpy()
    assert (st == 3).sum() >= 1
    start = np.clip(shifted.cpu().numpy().astype(F), F(-BOUND), F(BOUND))
    moved_before_stop = np.any(want["positions"] != start, axis=1)
    first = (st == 3) & ~moved_before_stop                                           # stopped at the first step: still at clamp(input)
    assert first.any() and np.array_equal(got["positions"].cpu().numpy()[first], start[first])
    # (b) a field whose table and weight matrices are zero: the sdf is the constant b2[0], there is no gradient to follow
    p = env["p"]
    zero = lambda k: torch.zeros_like(f.t[k])
    assert abs(float(f.t["b2"][0])) > TOL
    zf = nsr_ops.Field(zero("table"), [int(o) for o in p["offsets"]], float(p["per_level_scale"]), 16, zero("W1"), f.t["b1"], zero("W2"), f.t["b2"],
                       zero("Wc1"), zero("Wc2"), zero("Wc3"))
    z = nsr_ops.mesh_vertex_attrs(zf, v, BOUND, EPS, refine_steps=3, tol=TOL, max_move=h)
    assert bool((z["status"] == 2).all()) and torch.equal(z["positions"], v.float().clamp(-BOUND, BOUND)) and bool((z["normals"] == 0).all())
    assert bool((z["sdf"] == f.t["b2"][0]).all()) and all(bool(torch.isfinite(t.float()).all()) for t in z.values())
    # (c) a tolerance everything meets
    c = nsr_ops.mesh_vertex_attrs(f, v, BOUND, EPS, refine_steps=3, tol=1.0, max_move=h)
    assert bool((c["status"] == 0).all()) and torch.equal(c["positions"], v.float().clamp(-BOUND, BOUND))
    # (d) another level: the surface sdf = 0.01 is extract_geometry's threshold -0.01
    m = net.extract_colored_mesh(BOUND, 48, threshold=-0.01, return_torch=True)
    v01 = net.extract_geometry(BOUND, 48, threshold=-0.01, return_torch=True)[0]
    want = restate(oracle, env["of_net"], v01.cpu().numpy(), 3, h, target=0.01)
    same(dict(positions=m["vertices"].float(), normals=m["normals"], sdf=m["sdf"], rgb=m["colors"], status=m["status"]), want, "target 0.01")
    assert np.abs(want["sdf"] - F(0.01)).max() <= 1e-4 and float((m["sdf"] - 0.01).abs().max()) <= 1e-4


def test_view_directions(oracle):
    from avatarcraft_amd import nsr_ops
    from tests.test_gpu_viewdirs import viewdirs_net
    g = load_golden("viewdirs.npz")
    net = viewdirs_net(g)
    of = oracle_twin(oracle, net, g["offsets"], g["per_level_scale"])
    assert of.has_viewdirs and net._field().has_viewdirs
    v = net.extract_geometry(BOUND, 24, return_torch=True)[0]
    assert v.shape[0] > 16
    h = cell(24)
    got = nsr_ops.mesh_vertex_attrs(net._field(), v, BOUND, EPS, refine_steps=3, tol=TOL, max_move=h)
    same(got, restate(oracle, of, v.cpu().numpy(), 3, h), "dirs = -normal")
    d = np.random.RandomState(5).normal(size=(v.shape[0], 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    got = nsr_ops.mesh_vertex_attrs(net._field(), v, BOUND, EPS, refine_steps=3, tol=TOL, max_move=h, dirs=torch.from_numpy(d).to(DEV))
    same(got, restate(oracle, of, v.cpu().numpy(), 3, h, dirs=d), "explicit dirs")
    m = net.extract_colored_mesh(BOUND, 24, return_torch=True)
    assert float(m["colors"].min()) >= 0.0 and float(m["colors"].max()) <= 1.0


def test_geometry_only_mode(env):
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    net = env["net"]
    v = net.extract_geometry(BOUND, 48, return_torch=True)[0]
    full = nsr_ops.mesh_vertex_attrs(net._field(), v, BOUND, EPS, refine_steps=3, tol=TOL, max_move=cell(48))
    for field in (net._field(), net._field_sdf_only()):
        geo = nsr_ops.mesh_vertex_attrs(field, v, BOUND, EPS, refine_steps=3, tol=TOL, max_move=cell(48), want_rgb=False)
        assert geo["rgb"] is None and all(torch.equal(geo[k], full[k]) for k in ("positions", "normals", "sdf", "status"))
    # a model with the default SDF side and another colour network: geometry and normals, and a named reason for the colours
    torch.manual_seed(0)
    other = NeRFNetwork(hidden_dim_color=32)
    other.load_state_dict({k: t for k, t in net.state_dict().items() if not k.startswith("color_net")}, strict=False)
    other = other.to(DEV).eval()
    assert other._sdf_supported() and not other._fused_supported()
    m = other.extract_colored_mesh(BOUND, 48, colors=False, return_torch=True)
    assert "colors" not in m and torch.equal(m["vertices"].float(), full["positions"]) and torch.equal(m["normals"], full["normals"])
    with pytest.raises(RuntimeError, match="colour side"):
        other.extract_colored_mesh(BOUND, 48)


def test_projection_improves_the_mesh_and_keeps_its_topology(env, tmp_path):
    net = env["net"]
    vt = net.extract_geometry(BOUND, 48, return_torch=True)
    v0, t0 = (x.cpu().numpy() for x in vt)
    m = net.extract_colored_mesh(BOUND, 48)
    assert set(m) == {"vertices", "triangles", "normals", "colors", "sdf", "status"} and all(isinstance(x, np.ndarray) for x in m.values())
    assert np.abs(m["sdf"]).max() <= 1e-4
    assert m["triangles"].dtype == np.int32 and np.array_equal(m["triangles"], t0)
    fn = lambda v: np.cross(v[t0[:, 1]] - v[t0[:, 0]], v[t0[:, 2]] - v[t0[:, 0]])
    n0, n1 = fn(v0), fn(m["vertices"])
    assert ((n0 * n1).sum(1) > 0).all()                                              # every triangle keeps its orientation
    vn = np.zeros_like(v0)
    for k in range(3):
        np.add.at(vn, t0[:, k], n1)                                                  # area-weighted face normals gathered at the vertices
    assert ((vn * m["normals"]).sum(1) > 0).all()
    assert not np.isin(m["status"], (2, 3)).any()
    assert m["colors"].dtype == np.float32 and m["colors"].min() >= 0.0 and m["colors"].max() <= 1.0
    assert m["vertices"].dtype == np.float64 and m["normals"].dtype == np.float32
    mt = net.extract_colored_mesh(BOUND, 48, return_torch=True)
    assert all(x.is_cuda for x in mt.values()) and mt["vertices"].dtype == torch.float64
    assert np.array_equal(mt["vertices"].cpu().numpy(), m["vertices"]) and np.array_equal(m["vertices"], m["vertices"].astype(F).astype(np.float64))
    from avatarcraft_amd import nsr_ops
    a = nsr_ops.mesh_vertex_attrs(net._field(), vt[0], BOUND, EPS, refine_steps=3, tol=TOL, max_move=cell(48))
    assert torch.equal(mt["vertices"], a["positions"].double()) and torch.equal(mt["colors"], a["rgb"])
    # ... and written down: the driver's file holds this mesh (the layout itself is pinned on the CPU tier, tests/test_mesh_export_host.py)
    from avatarcraft_amd import drivers
    from tests.test_mesh_export_host import read_ply
    d = drivers.export_mesh(net, str(tmp_path / "avatar.ply"), bound=BOUND, resolution=48)
    props, vert, faces, _ = read_ply(str(tmp_path / "avatar.ply"))
    assert len(props) == 9 and np.array_equal(faces, t0) and np.array_equal(d["vertices"], m["vertices"])
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), m["vertices"].astype(F))
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), np.round(m["colors"].astype(np.float64) * 255.0).astype(np.uint8))


def test_export_at_the_references_resolution(env):
    """extract_geometry(NSR_BOUND, 512) is the reference's one call (stylize.py:267); here with normals and colours on it"""
    net = env["net"]
    m = net.extract_colored_mesh(BOUND, 512, return_torch=True)
    V, T = m["vertices"].shape[0], m["triangles"].shape[0]
    assert V > 50000 and T > 100000 and m["vertices"].shape == (V, 3) and m["normals"].shape == (V, 3) and m["colors"].shape == (V, 3)
    assert m["sdf"].shape == (V,) and m["status"].shape == (V,) and m["status"].dtype == torch.uint8
    assert all(bool(torch.isfinite(m[k]).all()) for k in ("vertices", "normals", "colors", "sdf"))
    st = m["status"]
    hist = torch.bincount(st.long(), minlength=4).tolist()
    print("512^3: V =", V, "status histogram", hist, "max |sdf| over status 0:", float(m["sdf"][st == 0].abs().max()))
    assert hist[2] + hist[3] < 1e-3 * V, hist
    assert float(m["sdf"][st == 0].abs().max()) <= 1e-5
