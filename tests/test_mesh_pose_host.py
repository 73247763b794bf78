"""CPU tier of the mesh posing (ac_mesh_bind / ac_mesh_pose, csrc/mesh_pose.hip): the definitions of include/avatarcraft_hip.h restated in numpy fp64 around
the CPU oracle's closest-face search (tests/mesh_pose_cases.py) behave as the design says, and the host-side pieces around them (geometry.canonical_guide,
geometry.skin_weights, drivers.export_animation's files).  The GPU tier (tests/test_gpu_mesh_pose.py) compares the kernels with the same restatement bit for bit."""
import os

import numpy as np
import pytest

from tests import mesh_pose_cases as MC

# measured with restate_pose on the smooth guide (482 vertices / 960 faces), 960 offset points, tol 1e-5, max-norm residual of the returned position:
#   frame  iters  median    p99       status histogram [0 within tol, 1 iters used up, 2 not finite]
RECORDED = {(5, 0): (3.103e-4, 1.532e-2, [60, 900, 0]), (5, 2): (5.467e-6, 1.198e-3, [623, 337, 0]), (5, 3): (3.805e-6, 5.374e-4, [764, 196, 0]),
            (12, 0): (3.632e-4, 9.984e-3, [81, 879, 0]), (12, 2): (5.624e-6, 1.270e-3, [629, 331, 0]), (12, 3): (3.610e-6, 1.138e-3, [825, 135, 0])}


@pytest.fixture(scope="module")
def bound_case(oracle):
    cs = MC.case()
    return cs, MC.restate_bind(oracle, cs["points"], cs["guide"], cs["faces"])


@pytest.mark.parametrize("frame", [5, 12])
def test_fixed_point_iteration_contracts(oracle, bound_case, frame):
    """restate_pose on frames 5 and 12 at iters 0, 2, 3 (tol 1e-5).  Recorded (max-norm residual; median / p99 / status histogram):
        frame 5:  iters 0: 3.10e-4 / 1.53e-2 / [60, 900, 0]   iters 2: 5.47e-6 / 1.20e-3 / [623, 337, 0]   iters 3: 3.81e-6 / 5.37e-4 / [764, 196, 0]
        frame 12: iters 0: 3.63e-4 / 9.98e-3 / [81, 879, 0]   iters 2: 5.62e-6 / 1.27e-3 / [629, 331, 0]   iters 3: 3.61e-6 / 1.14e-3 / [825, 135, 0]
    (the median stops falling near 4e-6 because a vertex stops as soon as it is within tol; a handful of points whose closest face flips between iterates keep
    0.7 - 0.8 cm: they are reported through status 1 and residual, not hidden)"""
    cs, bind = bound_case
    got = {}
    for iters in (0, 2, 3):
        r = MC.restate_pose(oracle, cs["points"], cs["normals"], bind, cs["verts"][frame], cs["faces"], cs["Ts"][frame], iters, 1e-5)
        res = r["residual"].astype(np.float64)
        got[iters] = (float(np.median(res)), float(np.percentile(res, 99)), np.bincount(r["status"], minlength=3).tolist())
        print(f"frame {frame} iters {iters}: median {got[iters][0]:.3e} p99 {got[iters][1]:.3e} status {got[iters][2]}")
        assert r["evaluations"] == iters + 1 and np.isfinite(r["positions"]).all() and (r["mask"] == 1).all()
        assert ((r["status"] == 0) == (res <= np.float64(np.float32(1e-5)))).all()
        assert np.abs(np.linalg.norm(r["normals"].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    for iters in (0, 2, 3):
        med, p99, hist = RECORDED[(frame, iters)]
        assert got[iters][0] <= 2.0 * med and got[iters][1] <= 2.0 * p99, (iters, got[iters])
        # (the guide comes from numpy's sin / cos: a last-place difference on another machine moves residuals by ~1e-7 of a 1e-5 tolerance, a vertex or two)
        assert abs(got[iters][2][0] - hist[0]) <= 10 and got[iters][2][2] == 0 and sum(got[iters][2]) == 960, (iters, got[iters])
    assert got[2][0] <= got[0][0] / 5.0 and got[3][2][0] > got[2][2][0] > got[0][2][0]


@pytest.mark.parametrize("frame", [5, 12])
def test_posing_the_guides_own_vertices_gives_the_posed_guide(oracle, frame):
    cs = MC.case()
    g = cs["guide"]
    bind = MC.restate_bind(oracle, g, g, cs["faces"])
    assert bind["dist2"].max() == 0.0 and np.abs(np.sort(bind["bary"], axis=1) - np.array([0.0, 0.0, 1.0])).max() <= 1e-12      # one-hot up to rounding
    r = MC.restate_pose(oracle, g, None, bind, cs["verts"][frame], cs["faces"], cs["Ts"][frame], 3, 1e-5)
    assert np.abs(r["positions"].astype(np.float64) - cs["verts"][frame]).max() <= 1e-5
    assert (r["status"] == 0).all() and r["residual"].max() <= 1e-5 and r["normals"] is None
    r0 = MC.restate_pose(oracle, g, None, bind, cs["verts"][frame], cs["faces"], cs["Ts"][frame], 0, 1e-5)                       # ... at k = 0 already
    assert (r0["status"] == 0).all() and np.array_equal(r0["positions"], r["positions"])


def test_canonical_guide_is_frame_independent():
    from avatarcraft_amd.geometry import canonical_guide
    cs = MC.case()
    g0, g5, g12 = (canonical_guide(cs["verts"][f], cs["Ts"][f]) for f in (0, 5, 12))
    assert g0.dtype == np.float32 and g0.shape == (482, 3)
    assert np.abs(g0 - g5).max() <= 1e-6 and np.abs(g0 - g12).max() <= 1e-6
    # the definition, vertex by vertex
    i = 77
    want = (np.linalg.inv(cs["Ts"][5][i]) @ np.append(cs["verts"][5][i].astype(np.float64), 1.0))[:3].astype(np.float32)
    assert np.array_equal(g5[i], want)
    with pytest.raises(ValueError):
        canonical_guide(cs["verts"][0], cs["Ts"][0][:10])


def test_skin_weights_rows_sum_to_one(oracle, bound_case):
    from avatarcraft_amd.geometry import skin_weights
    cs, bind = bound_case
    rs = np.random.RandomState(4)
    w = rs.uniform(size=(482, 24)) ** 4
    w /= w.sum(1, keepdims=True)
    sw = skin_weights(bind, cs["faces"], w)
    assert sw.shape == (960, 24) and np.abs(sw.sum(1) - 1.0).max() <= 1e-6
    k = 123
    tri = cs["faces"][bind["face_id"][k]]
    assert np.allclose(sw[k], (bind["bary"][k][:, None] * w[tri]).sum(0), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        skin_weights(dict(face_id=np.array([960]), bary=np.zeros((1, 3))), cs["faces"], w)


class _StubNet:
    """what export_animation asks of a net: one extraction, then pose_mesh per frame"""

    def __init__(self):
        self.extracted, self.posed = [], []
        v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        t = np.array([[0, 2, 1], [0, 1, 3]], np.int32)
        self.mesh = dict(vertices=v, triangles=t, normals=np.tile(np.float32([0, 0, 1]), (4, 1)), colors=np.full((4, 3), 0.5, np.float32))

    def extract_textured_mesh(self, bound, resolution, **kw):
        self.extracted.append(("obj", bound, resolution, kw))
        uv = np.tile(np.array([[0.1, 0.1], [0.4, 0.1], [0.1, 0.4]]), (2, 1, 1))
        return dict(self.mesh, uv=uv, texture=np.full((8, 8, 3), 200, np.uint8))

    def extract_colored_mesh(self, bound, resolution, **kw):
        self.extracted.append(("ply", bound, resolution, kw))
        return dict(self.mesh)

    def pose_mesh(self, mesh, body_guide, verts, Ts=None, iters=3, tol=1e-5):
        self.posed.append((body_guide, np.asarray(verts).shape, np.asarray(Ts).shape, iters))
        out = dict(mesh)
        out.update(vertices=mesh["vertices"] + float(len(self.posed)), status=np.zeros(4, np.uint8), residual=np.zeros(4, np.float32), mask=np.ones(4, np.uint8))
        return out


def _body():
    from avatarcraft_amd import smpl as SM
    from tests.common import make_body
    verts, faces, _ = make_body(n_lat=6, n_lon=8)
    return SM.BodyModel.synthetic(seed=2, n_verts=verts.shape[0], faces=faces, v_template=verts), verts.shape[0]


def test_export_animation_files_share_one_texture(tmp_path):
    from avatarcraft_amd import drivers as DR
    bm, nv = _body()
    poses = (np.random.RandomState(1).normal(size=(3, 72)) * 0.2).astype(np.float32)
    net = _StubNet()
    pat = str(tmp_path / "walk_%04d.obj")
    frames = list(DR.export_animation(net, bm, poses=poses, out_pattern=pat, resolution=16, iters=2, device="cpu", texture_size=8))
    assert [i for i, _ in frames] == [0, 1, 2]
    assert net.extracted == [("obj", DR.NSR_BOUND, 16, dict(texture_size=8))]                       # extracted and baked once
    assert len(net.posed) == 3 and all(p[0] is net.posed[0][0] for p in net.posed)                  # one guide dict: bound once
    guide = net.posed[0][0]
    assert guide["canonical"].shape == (nv, 3) and guide["canonical"].dtype == np.float32 and net.posed[0][1:] == ((nv, 3), (nv + 24, 4, 4), 2)
    assert sorted(os.listdir(tmp_path)) == ["walk.mtl", "walk.png", "walk_0000.obj", "walk_0001.obj", "walk_0002.obj"]
    assert "map_Kd walk.png" in open(tmp_path / "walk.mtl").read()
    for k in range(3):
        lines = open(tmp_path / f"walk_{k:04d}.obj").read().splitlines()
        assert lines[0] == "mtllib walk.mtl" and lines[1] == "usemtl baked"
        assert lines[2] == "v %r %r %r" % (k + 1.0, k + 1.0, k + 1.0)                               # the frame's own vertices ...
        assert [l for l in lines if l.startswith("f ")] == ["f 1/1/1 3/2/3 2/3/2", "f 1/4/1 2/5/2 4/6/4"]      # ... on the same triangles and UVs
        assert frames[k][1]["triangles"] is frames[0][1]["triangles"] and frames[k][1]["uv"] is frames[0][1]["uv"]
    # vertex colours instead, sharded over two ranks
    net2 = _StubNet()
    os.makedirs(tmp_path / "ply")
    got = list(DR.export_animation(net2, bm, poses=poses, out_pattern=str(tmp_path / "ply" / "f%02d.ply"), resolution=16, device="cpu", rank=1, world=2))
    assert [i for i, _ in got] == [1] and os.listdir(tmp_path / "ply") == ["f01.ply"] and net2.extracted[0][0] == "ply"
    from tests.test_mesh_export_host import read_ply
    props, vert, faces, _ = read_ply(str(tmp_path / "ply" / "f01.ply"))
    assert len(props) == 9 and np.array_equal(faces, net2.mesh["triangles"]) and vert["x"][1] == 2.0 and vert["red"][0] == 128
    # shape interpolation takes the other branch of calc_local_trans
    net3 = _StubNet()
    got = list(DR.export_animation(net3, bm, shape_from=np.zeros((1, 10)), shape_to=np.ones((1, 10)), out_pattern=str(tmp_path / "s_%d.ply"), resolution=16,
                                   device="cpu", max_frames=2))
    assert [i for i, _ in got] == [0, 1]
    for bad in ("frame.obj", "frame_%04d.stl", "frame_%s_%d.obj"):
        with pytest.raises(ValueError):
            next(DR.export_animation(net, bm, poses=poses, out_pattern=str(tmp_path / bad), device="cpu"))


def test_the_new_entries_are_declared_and_bound():
    import ctypes
    from avatarcraft_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avatarcraft_hip.h")).read()
    for name in ("ac_mesh_bind", "ac_mesh_bind_scratch", "ac_mesh_pose", "ac_mesh_pose_scratch"):
        assert name in _lib.EXPORTS and f"{name}(" in hdr
    assert ctypes.sizeof(_lib.ac_mesh_pose_opts) == 8 and _lib.ac_mesh_pose_opts.tol.offset == 4
    assert "typedef struct ac_mesh_pose_opts { int32_t iters; float tol; } ac_mesh_pose_opts;" in hdr
