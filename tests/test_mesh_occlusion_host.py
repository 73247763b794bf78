"""CPU: ambient occlusion without the library or a GPU -- the kit and its refusals (avatarcraft_amd/mesh_occlusion.py), the numpy restatement of the kernel's
arithmetic (tests/mesh_occlusion_cases.py) on analytic distance fields, the ctypes mirrors of the two new structs, the file writers' new arguments and the
refusals of the front end that need no device."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.mesh_occlusion_cases import F, occluded, occlusion_reference


def test_default_kit():
    from avatarcraft_amd.mesh_occlusion import occlusion_kit
    for K, J in ((8, 4), (1, 1), (32, 16), (5, 3)):
        kit = occlusion_kit(0.25, directions=K, steps=J)
        d, w, t = kit["dirs"], kit["weights"], kit["dists"]
        assert d.dtype == w.dtype == t.dtype == np.float32 and d.shape == (K, 3) and w.shape == (K,) and t.shape == (J,)
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6                       # unit directions
        assert d[0, 2] == np.float32(math.sqrt(1.0 - 0.5 / K)) and (np.diff(d[:, 2]) < 0).all() and d[-1, 2] >= 0.05      # lz descending from sqrt(1 - 0.5 / K)
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6 and (w == np.float32(1.0 / K)).all()
        assert np.array_equal(t, (0.25 * (np.arange(J) + 1.0) / J).astype(np.float32)) and t[-1] == np.float32(0.25)
        assert kit["gain"] == 1.0 and kit["level"] == 0.0
    i = np.arange(8) + 0.5
    want = np.stack([np.sqrt(i / 8) * np.cos(i * math.pi * (3 - math.sqrt(5))), np.sqrt(i / 8) * np.sin(i * math.pi * (3 - math.sqrt(5))), np.sqrt(1 - i / 8)], 1)
    assert np.array_equal(occlusion_kit(1.0)["dirs"], want.astype(np.float32))
    # explicit tables replace the defaults
    kit = occlusion_kit(dirs=[[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]], weights=[0.25, 0.75], dists=[0.1, 0.3], gain=2.0, level=0.01)
    assert kit["dirs"].shape == (2, 3) and kit["weights"].tolist() == [0.25, 0.75] and kit["dists"].dtype == np.float32 and kit["gain"] == 2.0 and kit["level"] == 0.01


def test_kit_refusals():
    from avatarcraft_amd.mesh_occlusion import check_kit, occlusion_kit, resolve_kit
    up = [[0.0, 0.0, 1.0]]
    bad = [dict(radius=0.1, directions=33), dict(radius=0.1, directions=0), dict(radius=0.1, directions=2.5), dict(radius=0.1, steps=17), dict(radius=0.1, steps=0),
           dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=None), dict(radius="wide"),
           dict(radius=0.1, gain=0.0), dict(radius=0.1, gain=-1.0), dict(radius=0.1, gain=float("inf")), dict(radius=0.1, level=float("nan")),
           dict(radius=0.1, dirs=[[0.0, 0.0, 1.0]] * 33), dict(radius=0.1, dirs=[[math.sqrt(1 - 1e-4), 0.0, 0.01]]), dict(radius=0.1, dirs=[[0.0, 0.0, 1.01]]),
           dict(radius=0.1, dirs=[[0.0, 0.0, -1.0]]), dict(radius=0.1, dirs=[[float("nan"), 0.0, 1.0]]), dict(radius=0.1, dirs=[0.0, 0.0, 1.0]),
           dict(radius=0.1, dirs=up, weights=[0.5]), dict(radius=0.1, dirs=up, weights=[1.0, 0.0]), dict(radius=0.1, dirs=up * 2, weights=[1.5, -0.5]),
           dict(radius=0.1, dirs=up, weights=[1.0 + 1e-4]), dict(dists=[0.2, 0.1]), dict(dists=[0.1, 0.1]), dict(dists=[0.0, 0.1]), dict(dists=[-0.1]),
           dict(dists=[float("inf")]), dict(dists=[]), dict(dists=np.linspace(0.01, 0.2, 17))]
    for kw in bad:
        with pytest.raises(ValueError, match="occlusion_kit"):
            occlusion_kit(**kw)
    good = occlusion_kit(0.1)
    for key, val in (("gain", 0.0), ("dists", good["dists"][::-1]), ("weights", good["weights"] * 2), ("dirs", -good["dirs"])):
        with pytest.raises(ValueError, match="occlusion_kit"):
            check_kit(dict(good, **{key: val}))
    with pytest.raises(ValueError, match="occlusion_kit"):
        check_kit({k: v for k, v in good.items() if k != "level"})
    # the spec of the front end's occlusion= argument
    assert np.array_equal(resolve_kit(True, 1.6)["dists"], occlusion_kit(0.16)["dists"]) and resolve_kit(True, 1.6, level=0.02)["level"] == 0.02
    k = resolve_kit(dict(directions=4, steps=2, gain=1.5), 2.0, level=-0.5)
    assert k["dirs"].shape == (4, 3) and k["dists"].tolist() == [np.float32(0.1), np.float32(0.2)] and k["gain"] == 1.5 and k["level"] == -0.5
    assert resolve_kit(dict(good, level=0.25), 1.6, level=0.0)["level"] == 0.25                           # a kit is passed as is
    for spec in (False, 1, "yes", dict(directions=33), dict(radios=0.1), dict(good, gain=0.0)):
        with pytest.raises(ValueError, match="occlusion"):
            resolve_kit(spec, 1.6)


def _frame_is_orthonormal(n):
    """the frame of the restatement, probed through a kit of one direction: the tap of direction l at distance 1 lands at l's image"""
    out = []
    for l in ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]):
        seen = []
        kit = dict(dirs=np.array([l], F), weights=np.array([1.0], F), dists=np.array([1.0], F), gain=1.0, level=0.0)
        occlusion_reference(lambda q: (seen.append(q.copy()), np.zeros(len(q), F))[1], np.zeros((1, 3), F), np.array([n], F), 8.0, kit)
        out.append(seen[0][0])
    return np.array(out, np.float64)


def test_restatement_on_analytic_fields():
    from avatarcraft_amd.mesh_occlusion import occlusion_kit
    rs = np.random.RandomState(3)
    normals = rs.normal(size=(64, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    normals = np.concatenate([normals, [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0.6, 0, -0.8], [1e-4, 0, -math.sqrt(1 - 1e-8)]]]).astype(F)
    assert (normals[:, 2] < 0).sum() > 10 and (normals[:, 2] > 0).sum() > 10
    for n in normals[::7].tolist() + [[0.0, 0.0, -1.0]]:
        M = _frame_is_orthonormal(n)                                                   # rows: T, U, n
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-6 and np.linalg.det(M) > 0.999 and np.allclose(M[2], n, atol=1e-7)
    # a plane through the origin under every normal: the true distance is q . n.  The points are the origin itself, where a tap q = p + t w is formed without
    # rounding p + .: at |p| ~ 1 that sum alone is off by 6e-8, which the division by h = t lz (2.5e-2 and less) turns into more than the 1e-6 asked for here
    points = np.zeros((len(normals), 3), F)
    bound = 4.0
    n64 = normals.astype(np.float64)
    for kit in (occlusion_kit(0.4), occlusion_kit(0.4, directions=32, steps=16, gain=1.5), occlusion_kit(0.05, directions=1, steps=1)):
        got = np.array([occlusion_reference(lambda q: (q.astype(np.float64) @ n64[i]).astype(F), points[i:i + 1], normals[i:i + 1], bound, kit)[0]
                        for i in range(len(points))])
        assert got.dtype == F and got.min() >= 1.0 - 1e-6 and got.max() <= 1.0, (got.min(), got.max())
    # the bottom of a narrow spherical pit (free space: the inside of a ball of radius 0.1 resting on the point) scores lower than a point on the plane
    kit = occlusion_kit(0.4)
    for n in ([0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.6, 0.0, 0.8]):
        n64 = np.array(n)
        pit = lambda q: (0.1 - np.linalg.norm(q.astype(np.float64) - 0.1 * n64, axis=1)).astype(F)
        flat = lambda q: (q.astype(np.float64) @ n64).astype(F)
        o_pit = occlusion_reference(pit, np.zeros((1, 3), F), np.array([n], F), bound, kit)[0]
        o_flat = occlusion_reference(flat, np.zeros((1, 3), F), np.array([n], F), bound, kit)[0]
        assert o_flat >= 1.0 - 1e-6 and o_pit < 0.5 * o_flat, (o_pit, o_flat)
    # a NaN-valued field: exactly 0; inactive and non-finite rows: 0 and never evaluated
    nan = lambda q: np.full(len(q), np.nan, F)
    assert not occlusion_reference(nan, points, normals, bound, kit).any()
    seen = []
    def flat_z(q):
        seen.append(len(q))
        return q[:, 2]
    up = np.tile(np.array([[0.0, 0.0, 1.0]], F), (6, 1))
    pts = np.zeros((6, 3), F); pts[1, 0] = np.inf; up[2, 1] = np.nan
    mask = np.array([1, 1, 1, 0, 1, 1], bool)
    o = occlusion_reference(flat_z, pts, up, bound, kit, active=mask)
    assert o[[1, 2, 3]].tolist() == [0.0, 0.0, 0.0] and (o[[0, 4, 5]] >= 1.0 - 1e-6).all() and set(seen) == {3}
    assert not occlusion_reference(flat_z, pts, up, bound, kit, active=np.zeros(6, bool)).any() and set(seen) == {3}
    # the level: the plane z = 0.25 seen as the level set 0.25 of the field z
    lifted = np.zeros((1, 3), F); lifted[0, 2] = 0.25
    assert occlusion_reference(lambda q: q[:, 2], lifted, up[:1], bound, dict(kit, level=0.25))[0] >= 1.0 - 1e-6
    assert occlusion_reference(lambda q: q[:, 2], lifted, up[:1], bound, dict(kit, level=0.5))[0] < 0.7
    # taps that would leave the cube are clamped onto it
    qs = []
    occlusion_reference(lambda q: (qs.append(q), q[:, 2])[1], np.full((1, 3), 3.9, F), up[:1], bound, kit)
    assert max(float(q.max()) for q in qs) == 4.0


def test_struct_mirrors_match_the_header():
    """sizeof and offsets as include/avatarcraft_hip.h lays the two structs out on an LP64 target: two int32, three pointers, two floats | seven pointers"""
    from avatarcraft_amd import _lib
    o = _lib.ac_occlusion_opts
    assert [f[0] for f in o._fields_] == ["n_dirs", "n_steps", "dirs", "weights", "dists", "gain", "level"]
    assert ctypes.sizeof(o) == 40 and [getattr(o, f[0]).offset for f in o._fields_] == [0, 4, 8, 16, 24, 32, 36]
    b = _lib.ac_bake_out
    assert [f[0] for f in b._fields_] == ["rgb", "owner", "normals", "positions", "sdf", "status", "occlusion"]
    assert ctypes.sizeof(b) == 56 and [getattr(b, f[0]).offset for f in b._fields_] == [0, 8, 16, 24, 32, 40, 48]
    assert "ac_field_occlusion" in _lib.EXPORTS and "ac_mesh_bake_maps" in _lib.EXPORTS
    assert len(_lib._SIGS["ac_field_occlusion"][0]) == 9 and len(_lib._SIGS["ac_mesh_bake_maps"][0]) == 10


def test_file_writers(tmp_path):
    from avatarcraft_amd.geometry import atlas_layout, save_obj, save_ply
    from tests.test_mesh_export_host import read_ply
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float64)
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    n = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (4, 1))
    c = np.array([[0.0, 0.5, 1.0], [1.0, 0.2, 0.5], [0.25, 0.75, 1.0], [0.0, 0.0, 0.0]], np.float32)
    q = np.array([0.0, 0.25, 0.8125, 1.0], np.float32)
    save_ply(str(tmp_path / "a.ply"), v, t, normals=n, colors=c)
    save_ply(str(tmp_path / "b.ply"), v, t, normals=n, colors=c, quality=None)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes() and b"quality" not in (tmp_path / "a.ply").read_bytes()
    assert read_ply(str(tmp_path / "a.ply"))[1].dtype.itemsize == 27
    for quality in (q, torch.from_numpy(q), q.astype(np.float64)):
        save_ply(str(tmp_path / "q.ply"), v, t, normals=n, colors=c, quality=quality)
        props, vert, faces, _ = read_ply(str(tmp_path / "q.ply"))
        assert props[-4:] == ["uchar red", "uchar green", "uchar blue", "float quality"] and vert.dtype.itemsize == 31
        assert np.array_equal(vert["quality"], q) and np.array_equal(faces, t) and np.array_equal(vert["nx"], n[:, 0])
        plain = read_ply(str(tmp_path / "a.ply"))[1]
        assert all(np.array_equal(vert[k], plain[k]) for k in plain.dtype.names)
    save_ply(str(tmp_path / "g.ply"), v, t, quality=q)
    assert read_ply(str(tmp_path / "g.ply"))[0] == ["float x", "float y", "float z", "float quality"]
    uv = atlas_layout(4, 32)["uv"]
    save_obj(str(tmp_path / "a.obj"), v, t, uv, normals=n, texture="a.png")
    before = (tmp_path / "a.obj").read_bytes(), (tmp_path / "a.mtl").read_bytes()
    save_obj(str(tmp_path / "a.obj"), v, t, uv, normals=n, texture="a.png", occlusion_texture=None)
    assert before == ((tmp_path / "a.obj").read_bytes(), (tmp_path / "a.mtl").read_bytes())
    assert (tmp_path / "a.mtl").read_text() == "newmtl baked\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd a.png\n"
    save_obj(str(tmp_path / "c.obj"), v, t, uv, normals=n, texture="a.png", occlusion_texture="a_ao.png")
    assert (tmp_path / "c.obj").read_text().replace("mtllib c.mtl", "mtllib a.mtl") == (tmp_path / "a.obj").read_text()
    assert (tmp_path / "c.mtl").read_text() == (tmp_path / "a.mtl").read_text() + "map_Ka a_ao.png\n"
    with pytest.raises(ValueError, match="occlusion_texture"):
        save_obj(str(tmp_path / "d.obj"), v, t, uv, occlusion_texture="a_ao.png")


def test_front_end_refusals_without_a_device():
    from avatarcraft_amd import mesh_occlusion
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork()                                                                # on the CPU
    for call in (net.extract_colored_mesh, net.extract_textured_mesh):
        for spec in (dict(directions=33), dict(gain=0.0), "yes", dict(dists=[0.2, 0.1])):
            with pytest.raises(ValueError, match="occlusion"):                         # the kit is refused before the model is even looked at
                with occluded(net, spec):
                    call(1.6, 16)
        with pytest.raises(RuntimeError, match="on the GPU"):
            with occluded(net, True):
                call(1.6, 16)
    rays = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="render_surface_posed: occlusion= is refused"):
        net.render_surface_posed(rays, rays, 1.6, None, None, None, occlusion=True)
    with pytest.raises(ValueError, match="occlusion"):
        net.render_surface(rays, rays, 1.6, occlusion=dict(steps=0))
    with pytest.raises(RuntimeError, match="on the GPU"):
        net.render_surface(rays, rays, 1.6, occlusion=True)
    kit = mesh_occlusion.occlusion_kit(0.1)
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="field_occlusion: points must be a CUDA tensor"):
        mesh_occlusion.field_occlusion(None, z, z, 1.6, kit)
    with pytest.raises(ValueError, match="occlusion_kit"):                             # the kit first
        mesh_occlusion.field_occlusion(None, z, z, 1.6, dict(kit, gain=0.0))
    with pytest.raises(RuntimeError, match="mesh_bake_maps: positions and triangles must be CUDA tensors"):
        mesh_occlusion.mesh_bake_maps(None, z, torch.zeros(1, 3, dtype=torch.int32), 64, 8, 1.6, kit=kit)
    with pytest.raises(ValueError, match="unknown outputs"):
        mesh_occlusion.mesh_bake_maps(None, z, torch.zeros(1, 3, dtype=torch.int32), 64, 8, 1.6, want=("rgb", "depth"))
