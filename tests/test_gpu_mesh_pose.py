"""-m gpu: ac_mesh_bind / ac_mesh_pose (csrc/mesh_pose.hip) and what stands on them -- nsr_ops.mesh_bind, nsr_ops.mesh_pose, NeRFNetwork.pose_mesh.
Every output is compared BIT FOR BIT with restate_bind / restate_pose (tests/mesh_pose_cases.py): the definitions of include/avatarcraft_hip.h in numpy fp64,
in the header's operation order, around the CPU oracle's closest-face search.  The case is the smooth synthetic guide (482 vertices, 960 faces) with 960 points
-3 .. +6 cm off its faces; what the iteration achieves there is recorded on the CPU tier (tests/test_mesh_pose_host.py)."""
import numpy as np
import pytest
import torch

from tests import mesh_pose_cases as MC
from tests.test_gpu_model import golden_net, DEV

pytestmark = pytest.mark.gpu
TOL = 1e-5
_REF = {}


def same_bits(got, want, what):
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    w = np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
    if g.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        g, w = np.ascontiguousarray(g).view(u), np.ascontiguousarray(w).view(u)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} values differ; first at {tuple(bad[0])}"


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                      # (a copy: the shared case is read-only)
    return t if dtype is None else t.to(dtype)


def ref_bind(oracle):
    if "bind" not in _REF:
        cs = MC.case()
        _REF["bind"] = MC.restate_bind(oracle, cs["points"], cs["guide"], cs["faces"])
    return _REF["bind"]


def ref_pose(oracle, frame, iters, tol=TOL):
    key = (frame, iters, tol)
    if key not in _REF:
        cs = MC.case()
        _REF[key] = MC.restate_pose(oracle, cs["points"], cs["normals"], ref_bind(oracle), cs["verts"][frame], cs["faces"], cs["Ts"][frame], iters, tol)
    return _REF[key]


@pytest.fixture(scope="module")
def env(oracle):
    """the case on the device, bound once through the culling structure; one WarpMesh per (frame, accel)"""
    from avatarcraft_amd import nsr_ops
    cs = MC.case()
    e = dict(cs=cs, pts=dev(cs["points"]), nrm=dev(cs["normals"]), guide=dev(cs["guide"]), faces=dev(cs["faces"]))
    e["bind"] = nsr_ops.mesh_bind(e["pts"], e["guide"], e["faces"])
    e["wm"] = {(f, a): nsr_ops.WarpMesh(cs["verts"][f].copy(), cs["faces"].copy(), cs["Ts"][f].copy(), DEV, accel=a) for f in (5, 12) for a in (True, False)}
    return e


def same_pose(got, want, what, n=None):
    sl = slice(None) if n is None else slice(0, n)
    for k in ("positions", "normals", "residual", "status", "mask"):
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            same_bits(got[k], want[k][sl], f"{what}: {k}")


def test_bind_bit_for_bit(oracle, env):
    from avatarcraft_amd import nsr_ops
    want = ref_bind(oracle)
    for accel in (True, False):
        got = env["bind"] if accel else nsr_ops.mesh_bind(env["pts"], env["guide"], env["faces"], accel=False)
        for k in ("face_id", "bary", "dist2"):
            same_bits(got[k], want[k], f"bind accel={accel}: {k}")
    assert got["bary"].dtype == torch.float64 and got["face_id"].dtype == torch.int32
    assert float((got["bary"].sum(1) - 1.0).abs().max()) <= 1e-12 and float(got["dist2"].max()) < 0.0601 ** 2


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("frame", [5, 12])
def test_pose_bit_for_bit_against_the_restatement(oracle, env, frame, accel):
    from avatarcraft_amd import nsr_ops
    for iters in (0, 1, 3):
        got = nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], env["wm"][(frame, accel)], iters=iters, tol=TOL)
        want = ref_pose(oracle, frame, iters)
        same_pose(got, want, f"frame {frame} iters {iters} accel {accel}")
    hist = np.bincount(want["status"], minlength=3)
    assert hist[0] > 700 and hist[2] == 0 and hist.sum() == 960, hist                # (a silently frozen iteration would show here)
    assert np.median(ref_pose(oracle, frame, 3)["residual"]) < np.median(ref_pose(oracle, frame, 0)["residual"]) / 5.0


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257, 960])
def test_wave_and_block_edges(oracle, env, V):
    """lane = vertex, 256 per workgroup: one lane, a wave short of one / full / one over, a workgroup plus one, and the whole set"""
    from avatarcraft_amd import nsr_ops
    pts, nrm = env["pts"][:V].contiguous(), env["nrm"][:V].contiguous()
    b = nsr_ops.mesh_bind(pts, env["guide"], env["faces"])
    want_b = ref_bind(oracle)
    for k in ("face_id", "bary", "dist2"):
        same_bits(b[k], want_b[k][:V], f"V={V} bind {k}")
    got = nsr_ops.mesh_pose(pts, nrm, b, env["wm"][(5, True)], iters=3, tol=TOL)
    same_pose(got, ref_pose(oracle, 5, 3), f"V={V}", n=V)
    assert all(t.shape[0] == V for t in got.values())


def test_stop_conditions(oracle, env):
    from avatarcraft_amd import nsr_ops
    cs, wm = env["cs"], env["wm"][(12, True)]
    # tol = 0: nobody stops early, every vertex takes exactly `iters` steps (iters + 1 evaluations; a step more or less would move the positions)
    for iters in (0, 2):
        got = nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], wm, iters=iters, tol=0.0)
        want = ref_pose(oracle, 12, iters, tol=0.0)
        assert want["evaluations"] == iters + 1 and (want["status"] == 1).all()
        same_pose(got, want, f"tol 0, iters {iters}")
    # a tolerance everything meets: status 0 at k = 0, the positions are the bound start p_0
    got = nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], wm, iters=3, tol=1e9)
    rb = ref_bind(oracle)
    p0 = MC.fwd(MC.blend(cs["Ts"][12], cs["faces"][rb["face_id"]], rb["bary"]), cs["points"])
    same_bits(got["positions"], p0, "huge tol: p_0")
    assert bool((got["status"] == 0).all())
    same_pose(got, ref_pose(oracle, 12, 0, tol=1e9), "huge tol == iters 0")
    # the guide's own vertices land on the posed guide, converged at k = 0
    g = env["guide"]
    gb = nsr_ops.mesh_bind(g, g, env["faces"])
    gp = nsr_ops.mesh_pose(g, None, gb, wm, iters=3, tol=TOL)
    assert bool((gp["status"] == 0).all()) and float(gp["residual"].max()) <= TOL
    assert float((gp["positions"] - wm.verts).abs().max()) <= 1e-5


def test_optional_buffers(env):
    from avatarcraft_amd import nsr_ops
    wm = env["wm"][(5, True)]
    full = nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], wm, iters=3, tol=TOL)
    bare = nsr_ops.mesh_pose(env["pts"], None, env["bind"], wm, iters=3, tol=TOL, want=())
    assert bare["normals"] is None and bare["residual"] is None and bare["status"] is None and bare["mask"] is None
    assert torch.equal(bare["positions"], full["positions"])
    some = nsr_ops.mesh_pose(env["pts"], None, env["bind"], wm, iters=3, tol=TOL, want=("status",))
    assert torch.equal(some["status"], full["status"]) and some["mask"] is None
    empty = nsr_ops.mesh_pose(env["pts"][:0].contiguous(), None, {k: t[:0].contiguous() for k, t in env["bind"].items()}, wm)
    assert empty["positions"].shape == (0, 3) and empty["status"].shape == (0,)
    again = nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], wm, iters=3, tol=TOL)
    assert all(torch.equal(again[k], full[k]) for k in full)


def test_refusals(env):
    from avatarcraft_amd import nsr_ops
    wm = env["wm"][(5, True)]
    with pytest.raises(RuntimeError, match="iters"):
        nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], wm, iters=17)
    with pytest.raises(RuntimeError, match="iters"):
        nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], wm, iters=-1)
    for bad_face in (-1, 960):
        b = dict(env["bind"], face_id=env["bind"]["face_id"].clone())
        b["face_id"][500] = bad_face
        with pytest.raises(RuntimeError, match="nothing was launched"):
            nsr_ops.mesh_pose(env["pts"], env["nrm"], b, wm)
    with pytest.raises(RuntimeError, match="CUDA"):
        nsr_ops.mesh_pose(env["pts"].cpu(), None, env["bind"], wm)
    with pytest.raises(RuntimeError, match="CUDA"):
        nsr_ops.mesh_bind(env["pts"].cpu(), env["guide"], env["faces"])
    bad = env["faces"].clone(); bad[3, 1] = 482
    with pytest.raises(RuntimeError, match="nothing was launched"):
        nsr_ops.mesh_bind(env["pts"], env["guide"], bad)
    # the device is fine afterwards
    ok = nsr_ops.mesh_pose(env["pts"], env["nrm"], env["bind"], wm, iters=1)
    assert bool(torch.isfinite(ok["positions"]).all())


MASKED_OUT_24 = 70          # of 184 vertices of the golden net's 24^3 mesh that frame 5 leaves farther than sqrt(0.05) from the capsule (measured on the oracle)


def test_pose_mesh_end_to_end(oracle, env, tmp_path):
    """extract_colored_mesh -> pose_mesh on the smooth body's frame 5: the golden field is a sphere, the guide a capsule -- most of the sphere lies where the posed
    renderer would draw it, the rest (farther than the mask threshold from the capsule) comes back flagged mask == 0: expected, and kept"""
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.geometry import save_ply
    from tests.test_mesh_export_host import read_ply
    cs = env["cs"]
    net, _ = golden_net()
    net.eval()
    mesh = net.extract_colored_mesh(1.6, 24, return_torch=True)
    V = mesh["vertices"].shape[0]
    assert V == 184
    guide = dict(faces=cs["faces"].copy(), canonical=cs["guide"].copy())
    posed = net.pose_mesh(mesh, guide, cs["verts"][5].copy(), cs["Ts"][5].copy())
    # == the op on the same inputs
    pts = mesh["vertices"].float().contiguous()
    b = nsr_ops.mesh_bind(pts, env["guide"], env["faces"])
    a = nsr_ops.mesh_pose(pts, mesh["normals"], b, env["wm"][(5, True)], iters=3, tol=TOL)
    assert torch.equal(posed["vertices"], a["positions"].double()) and torch.equal(posed["normals"], a["normals"])
    assert all(torch.equal(posed[k], a[k]) for k in ("residual", "status", "mask")) and all(torch.equal(guide["bind"][k], b[k]) for k in b)
    # == the restatement, and the flagged vertices are the ones the oracle flags
    rb = MC.restate_bind(oracle, pts.cpu().numpy(), cs["guide"], cs["faces"])
    want = MC.restate_pose(oracle, pts.cpu().numpy(), mesh["normals"].cpu().numpy(), rb, cs["verts"][5], cs["faces"], cs["Ts"][5], 3, TOL)
    same_pose(a, want, "golden 24^3")
    n_out = int((want["mask"] == 0).sum())
    print("24^3: masked-out vertices", n_out, "of", V, "status", np.bincount(want["status"], minlength=3).tolist())
    assert np.bincount(want["status"], minlength=3).tolist()[2] == 0
    assert n_out == MASKED_OUT_24 and int((posed["mask"] == 0).sum()) == n_out and 0 < n_out < V
    # untouched: the same objects; shapes and types
    assert posed["triangles"] is mesh["triangles"] and posed["colors"] is mesh["colors"] and posed["sdf"] is mesh["sdf"]
    assert posed["vertices"].shape == (V, 3) and posed["vertices"].dtype == torch.float64 and posed["normals"].shape == (V, 3)
    assert posed["residual"].shape == (V,) and posed["status"].dtype == torch.uint8 and posed["mask"].dtype == torch.uint8
    assert bool(torch.isfinite(posed["vertices"]).all()) and float((posed["normals"].norm(dim=1) - 1.0).abs().max()) < 1e-5
    assert float((posed["vertices"] - mesh["vertices"]).abs().max()) > 1e-2                      # the pose matters
    # a second frame reuses the binding; numpy in, numpy out
    kept = guide["bind"]
    mesh_np = {k: x.cpu().numpy() for k, x in mesh.items()}
    p12 = net.pose_mesh(mesh_np, guide, cs["verts"][12].copy(), cs["Ts"][12].copy())
    assert guide["bind"] is kept and isinstance(p12["vertices"], np.ndarray) and p12["triangles"] is mesh_np["triangles"]
    a12 = nsr_ops.mesh_pose(pts, mesh["normals"], b, env["wm"][(12, True)], iters=3, tol=TOL)
    assert np.array_equal(p12["vertices"], a12["positions"].double().cpu().numpy())
    # the PLY round trip
    path = str(tmp_path / "posed.ply")
    save_ply(path, posed["vertices"], posed["triangles"], normals=posed["normals"], colors=posed["colors"])
    props, vert, faces, _ = read_ply(path)
    assert len(props) == 9 and np.array_equal(faces, mesh["triangles"].cpu().numpy())
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), a["positions"].cpu().numpy())
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), a["normals"].cpu().numpy())


def test_export_animation_on_the_device(tmp_path):
    """drivers.export_animation with the real model: extracted and baked once, every frame posed through the WarpMesh that nsr_ops.warp_mesh_sequence prepared on
    its side stream == net.pose_mesh on the frame's arrays; the files share one material and one texture (the naming itself is pinned on the CPU tier)"""
    import os
    from avatarcraft_amd import drivers as DR, smpl as SM
    from avatarcraft_amd.geometry import canonical_guide
    from tests.common import make_body
    net, _ = golden_net()
    net.eval()
    verts, faces, _ = make_body(n_lat=10, n_lon=12)
    bm = SM.BodyModel.synthetic(seed=2, n_verts=verts.shape[0], faces=faces, v_template=verts)
    poses = (np.random.RandomState(1).normal(size=(3, 72)) * 0.2).astype(np.float32)
    frames = list(DR.export_animation(net, bm, poses=poses, out_pattern=str(tmp_path / "f_%03d.obj"), resolution=24, texture_size=256, device=DEV))
    assert [i for i, _ in frames] == [0, 1, 2]
    assert sorted(os.listdir(tmp_path)) == ["f.mtl", "f.png", "f_000.obj", "f_001.obj", "f_002.obj"]
    wv, Ts, _ = SM.calc_local_trans(bm, poses=poses)
    mesh = net.extract_textured_mesh(1.6, 24, texture_size=256)
    guide = dict(faces=np.asarray(bm.faces)[:, :3], canonical=canonical_guide(wv[0], Ts[0]))
    V = mesh["vertices"].shape[0]
    for i, posed in frames:
        want = net.pose_mesh(mesh, guide, wv[i], Ts[i])
        for k in ("vertices", "normals", "residual", "status", "mask"):
            assert isinstance(posed[k], np.ndarray) and np.array_equal(posed[k], want[k]), (i, k)
        assert np.array_equal(posed["triangles"], mesh["triangles"]) and np.array_equal(posed["uv"], mesh["uv"]) and np.array_equal(posed["texture"], mesh["texture"])
        assert posed["triangles"] is frames[0][1]["triangles"] and posed["vertices"].shape == (V, 3) and np.isfinite(posed["vertices"]).all()
        lines = open(tmp_path / f"f_{i:03d}.obj").read().splitlines()
        assert lines[0] == "mtllib f.mtl" and lines[2] == "v %r %r %r" % tuple(posed["vertices"][0].tolist())
        assert sum(l.startswith("v ") for l in lines) == V and sum(l.startswith("f ") for l in lines) == mesh["triangles"].shape[0]
    assert np.abs(frames[0][1]["vertices"] - frames[2][1]["vertices"]).max() > 1e-3                # the pose matters
    # vertex colours instead, one frame of two ranks
    got = list(DR.export_animation(net, bm, poses=poses, out_pattern=str(tmp_path / "c_%d.ply"), resolution=24, device=DEV, rank=1, world=3))
    assert [i for i, _ in got] == [1] and os.path.exists(tmp_path / "c_1.ply") and not os.path.exists(tmp_path / "c_0.ply")
    assert np.array_equal(got[0][1]["vertices"], frames[1][1]["vertices"]) and "colors" in got[0][1]
