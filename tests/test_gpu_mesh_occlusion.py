"""-m gpu: ambient occlusion on the device (csrc/mesh_occlusion.hip) -- mesh_occlusion.field_occlusion, mesh_bake_maps, and the front end around them
(extract_colored_mesh / extract_textured_mesh under NeRFNetwork.export_occlusion, render_surface(occlusion=...), drivers.export_mesh).  ac_field_occlusion is compared BIT FOR BIT with
tests/mesh_occlusion_cases.py, the header's procedure in numpy fp32 around the CPU oracle's Field.sdf; ac_mesh_bake_maps with ac_mesh_bake_texture for what they
share and with ac_field_occlusion for the rest.  Everything runs on the golden field's 24^3 mesh (184 vertices, 364 triangles; S = 128, c = 8: 11 648 owned texels)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_common import assert_bitwise
from tests.mesh_occlusion_cases import occluded, occlusion_reference
from tests.test_gpu_mesh_attrs import BOUND, EPS, TOL, F, cell, env, restate           # noqa: F401  (env: the module-scoped fixture, built once for the files that share it)
from tests.test_gpu_model import DEV
from tests.test_gpu_texture_bake import bake, meshes, reference as bake_ref           # noqa: F401

pytestmark = pytest.mark.gpu
_REF = {}
KITS = {"8x4": (8, 4, 0.4, 1.0, 0.0), "4x2": (4, 2, 0.4, 1.5, 0.0), "1x1": (1, 1, 0.2, 1.0, 0.0), "level": (4, 2, 0.4, 1.5, 0.02), "tight": (4, 2, 0.05, 1.5, 0.0)}


def make_kit(name):
    from avatarcraft_amd.mesh_occlusion import occlusion_kit
    K, J, radius, gain, level = KITS[name]
    return occlusion_kit(radius, directions=K, steps=J, gain=gain, level=level)


@pytest.fixture(scope="module")
def pn(env):
    """the 3-step mesh_vertex_attrs positions and normals of the 24^3 mesh, on the device and on the host -- computed once, never modified"""
    if "occ_pn" not in env:
        from avatarcraft_amd import nsr_ops
        a = nsr_ops.mesh_vertex_attrs(env["gf"], env["meshes"][24][0], BOUND, EPS, refine_steps=3, tol=TOL, max_move=cell(24))
        env["occ_pn"] = (a["positions"], a["normals"], a["positions"].cpu().numpy(), a["normals"].cpu().numpy())
        assert a["positions"].shape == (184, 3)
    return env["occ_pn"]


def ref(env, pn, name, flip=False):
    """the restatement around the oracle for one kit, at the mesh's vertices (flip: with the normals negated) -- computed once per kit"""
    key = (name, flip)
    if key not in _REF:
        sdf = lambda q: env["of"].sdf(q, BOUND)[:, 0]
        _REF[key] = occlusion_reference(sdf, pn[2], -pn[3] if flip else pn[3], BOUND, make_kit(name))
        _REF[key].setflags(write=False)
    return _REF[key]


def occ(env, p, n, kit, **kw):
    from avatarcraft_amd.mesh_occlusion import field_occlusion
    return field_occlusion(env["gf"], p, n, BOUND, kit, **kw)


@pytest.mark.parametrize("name", ["8x4", "4x2", "1x1", "level"])
def test_bit_for_bit_against_the_restatement(env, pn, name):
    kit = make_kit(name)
    got = occ(env, pn[0], pn[1], kit)
    want = ref(env, pn, name)
    print(name, "reference: min", want.min(), "max", want.max(), "exactly 1:", (want == 1).mean(), "exactly 0:", (want == 0).mean())
    assert got.dtype == torch.float32 and got.shape == (184,)
    assert_bitwise(got, want, f"kit {name}")
    assert torch.equal(occ(env, pn[0], pn[1], kit), got)                                # again: the same bits
    # the comparison is not vacuous: conditions on the REFERENCE
    if name == "8x4":
        assert want.min() > 0.2 and want.max() < 0.95
    if name == "4x2":
        assert 0.05 < (want == 1.0).mean() < 0.40                                      # the upper clamp is exercised
    if name == "level":
        assert not np.array_equal(want, ref(env, pn, "4x2"))


def test_negated_normals_saturate_at_zero(env, pn):
    """taps INTO the body: the lower clamp.  Bit for bit as well."""
    want = ref(env, pn, "tight", flip=True)
    print("tight, normals negated: exactly 0:", (want == 0).mean())
    assert (want == 0.0).mean() >= 0.90
    assert_bitwise(occ(env, pn[0], (-pn[1]).contiguous(), make_kit("tight")), want, "normals negated")


def test_tile_edges_and_inactive_rows(env, pn):
    from avatarcraft_amd import nsr_ops
    p, n = pn[0], pn[1]
    kit = make_kit("4x2")
    full = occ(env, p, n, kit)
    for m in (1, 15, 16, 17, 184):
        assert torch.equal(occ(env, p[:m].contiguous(), n[:m].contiguous(), kit), full[:m]), m
    # a whole inactive tile (rows 16..31) and a tile with one active lane (row 37 of 32..47)
    mask = torch.ones(184, dtype=torch.bool, device=DEV)
    mask[16:32] = False; mask[32:48] = False; mask[37] = True; mask[183] = False
    for act in (mask, mask.to(torch.uint8)):
        got = occ(env, p, n, kit, active=act)
        assert bool((got[~mask] == 0).all()) and torch.equal(got[mask], full[mask]) and int(mask.sum()) == 184 - 32
    assert not bool(occ(env, p, n, kit, active=torch.zeros(184, dtype=torch.bool, device=DEV)).any())
    # a NaN normal and an infinite coordinate, no mask: those rows store 0 and are never evaluated, every other row keeps its bits
    p2, n2 = p.clone(), n.clone()
    n2[5, 1] = float("nan"); p2[70, 0] = float("inf"); p2[71, 2] = float("-inf")
    got = occ(env, p2, n2, kit)
    bad = torch.zeros(184, dtype=torch.bool, device=DEV); bad[[5, 70, 71]] = True
    assert bool((got[bad] == 0).all()) and torch.equal(got[~bad], full[~bad])
    # a NaN hash table: every value is NaN, every tap counts as fully occluded
    f, q = env["gf"], env["p"]
    nf = nsr_ops.Field(torch.full_like(f.t["table"], float("nan")), [int(o) for o in q["offsets"]], float(q["per_level_scale"]), 16, f.t["W1"], f.t["b1"], f.t["W2"],
                       f.t["b2"], f.t["Wc1"], f.t["Wc2"], f.t["Wc3"])
    from avatarcraft_amd.mesh_occlusion import field_occlusion
    z = field_occlusion(nf, p, n, BOUND, kit)
    assert z.shape == (184,) and not bool(z.any()) and bool(torch.isfinite(z).all())
    # N = 0
    e = occ(env, p[:0].contiguous(), n[:0].contiguous(), kit)
    assert e.shape == (0,) and e.dtype == torch.float32
    # points outside the cube are clamped onto it first
    far = p * 4.0
    assert torch.equal(occ(env, far, n, kit), occ(env, far.clamp(-BOUND, BOUND), n, kit))


@pytest.mark.parametrize("steps", [0, 3])
def test_bake_maps(oracle, env, meshes, steps):
    from avatarcraft_amd.mesh_occlusion import field_occlusion, mesh_bake_maps
    pos, tris = meshes[24]
    S = 128
    tex = bake(env, pos, tris, S, 8, steps)
    run = lambda **kw: mesh_bake_maps(env["gf"], pos, tris, S, 8, BOUND, EPS, refine_steps=steps, tol=TOL, max_move=cell(24), **kw)
    shared = ("rgb", "owner", "normals", "sdf", "status")
    plain = run()
    assert plain["occlusion"] is None and all(torch.equal(plain[k], tex[k]) for k in shared)
    kit = make_kit("4x2")
    got = run(kit=kit)
    assert all(torch.equal(got[k], tex[k]) for k in shared)                            # the fused entry changes nothing it shares
    assert torch.equal(got["positions"], plain["positions"])
    want = bake_ref(oracle, env, meshes, 24, S, 8, steps)
    ys, xs = want["texels"]
    refined = restate(oracle, env["of"], want["start"], steps, cell(24))["positions"]
    assert_bitwise(got["positions"][torch.from_numpy(ys).to(DEV), torch.from_numpy(xs).to(DEV)], refined, "positions at the owned texels")
    owned = got["owner"] >= 0
    assert int(owned.sum()) == 11648
    o = field_occlusion(env["gf"], got["positions"].reshape(-1, 3), got["normals"].reshape(-1, 3), BOUND, kit, active=owned.reshape(-1))
    assert torch.equal(got["occlusion"].reshape(-1), o)
    for k in ("occlusion", "positions"):
        assert not bool(got[k][~owned].ne(0).any()), k
    inside = got["occlusion"][owned]
    assert float(inside.min()) >= 0.0 and float(inside.max()) <= 1.0 and float(inside.max()) > float(inside.min())
    assert torch.equal(run(kit=kit)["occlusion"], got["occlusion"])                     # again: the same bits
    lean = run(kit=kit, want=())                                                        # occlusion alone: no colour network
    assert all(lean[k] is None for k in ("rgb", "normals", "positions", "sdf", "status")) and torch.equal(lean["occlusion"], got["occlusion"])
    assert torch.equal(lean["owner"], got["owner"])


def test_corner_texels_equal_the_vertices(env, meshes):
    """at refine_steps=0 a UV corner's texel is the vertex itself: its occlusion is field_occlusion at that vertex, without the oracle"""
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.geometry import atlas_layout
    from avatarcraft_amd.mesh_occlusion import field_occlusion, mesh_bake_maps
    pos, tris = meshes[24]
    S, kit = 128, make_kit("4x2")
    got = mesh_bake_maps(env["gf"], pos, tris, S, 8, BOUND, EPS, kit=kit, refine_steps=0, tol=TOL, max_move=cell(24))
    va = nsr_ops.mesh_vertex_attrs(env["gf"], pos.double(), BOUND, EPS, refine_steps=0, tol=TOL, max_move=cell(24))
    ov = field_occlusion(env["gf"], va["positions"], va["normals"], BOUND, kit)
    uv = atlas_layout(tris.shape[0], S, 8)["uv"]
    x = torch.from_numpy(np.rint(uv[..., 0] * S - 0.5).astype(np.int64)).to(DEV)
    y = torch.from_numpy(np.rint((1.0 - uv[..., 1]) * S - 0.5).astype(np.int64)).to(DEV)
    assert torch.equal(got["occlusion"][y, x], ov[tris.long()]) and torch.equal(got["positions"][y, x], pos[tris.long()])


def test_through_the_model(env):
    from avatarcraft_amd.mesh_occlusion import field_occlusion
    from tests import surface_cases as S
    net = env["net"]
    kit = make_kit("4x2")
    f = net._field()
    plain = net.extract_colored_mesh(BOUND, 24, return_torch=True)
    with occluded(net, None):
        same_as_ever = net.extract_colored_mesh(BOUND, 24, return_torch=True)
    assert set(plain) == set(same_as_ever) == {"vertices", "triangles", "normals", "colors", "sdf", "status"}
    with occluded(net, kit):
        m = net.extract_colored_mesh(BOUND, 24, return_torch=True)
    assert set(m) == set(plain) | {"occlusion"} and all(torch.equal(m[k], plain[k]) and torch.equal(same_as_ever[k], plain[k]) for k in plain)
    assert m["occlusion"].dtype == torch.float32 and torch.equal(m["occlusion"], field_occlusion(f, m["vertices"].float(), m["normals"], BOUND, kit))
    with occluded(net, True):
        assert isinstance(net.extract_colored_mesh(BOUND, 24)["occlusion"], np.ndarray)
    # the textured mesh: one launch for the texels
    tp = net.extract_textured_mesh(BOUND, 24, texture_size=128, return_torch=True)
    with occluded(net, kit):
        t = net.extract_textured_mesh(BOUND, 24, texture_size=128, return_torch=True)
    assert set(t) == set(tp) | {"occlusion", "texel_occlusion", "occlusion_map"} and all(torch.equal(t[k], tp[k]) for k in tp)       # texture unchanged
    assert torch.equal(t["occlusion"], m["occlusion"]) and t["texel_occlusion"].shape == (128, 128) and t["occlusion_map"].dtype == torch.uint8
    assert torch.equal(t["occlusion_map"], torch.floor(t["texel_occlusion"].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8))
    assert not bool(t["texel_occlusion"][t["owner"] < 0].any()) and int(t["occlusion_map"].max()) > int(t["occlusion_map"][t["owner"] >= 0].min())
    # decimated and cleaned: the occlusion is taken at the final vertices
    with occluded(net, kit):
        d = net.extract_colored_mesh(BOUND, 24, return_torch=True, decimate=2, components="largest")
    assert d["vertices"].shape[0] < m["vertices"].shape[0] and d["occlusion"].shape == (d["vertices"].shape[0],)
    assert torch.equal(d["occlusion"], field_occlusion(f, d["vertices"].float(), d["normals"], BOUND, kit, active=d["status"] != 2))
    with occluded(net, kit):
        dt = net.extract_textured_mesh(BOUND, 24, texture_size=128, return_torch=True, decimate=2, components="largest")
    assert torch.equal(dt["occlusion"], d["occlusion"]) and dt["texel_occlusion"].shape == (128, 128)
    # another level: the kit takes the export's
    with occluded(net, dict(directions=4, steps=2, radius=0.4, gain=1.5)):
        lv = net.extract_colored_mesh(BOUND, 24, threshold=-0.01, return_torch=True)
    assert torch.equal(lv["occlusion"], field_occlusion(f, lv["vertices"].float(), lv["normals"], BOUND, dict(kit, level=0.01)))
    # the surface render
    o, dd = S.pinhole((0.3, 0.4, 2.6), n=16, fov=0.5)
    to, td = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (o, dd))
    with torch.no_grad():
        r0 = net.render_surface(to[None], td[None], BOUND)
        r = net.render_surface(to[None], td[None], BOUND, occlusion=kit)
        rb = net.render_surface(to[None], td[None], BOUND, occlusion=kit, max_ray_batch=100)
    assert set(r) == set(r0) | {"occlusion"} and all(torch.equal(r[k], r0[k]) for k in r0) and r["occlusion"].shape == (1, 256)
    hit = r["weight_sum"][:, 0] == 1
    assert 0 < int(hit.sum()) < 256 and bool((r["occlusion"][0][~hit] == 1).all()) and torch.equal(rb["occlusion"], r["occlusion"])
    assert torch.equal(r["occlusion"][0][hit], field_occlusion(f, r["position"][0], r["normal"], BOUND, kit)[hit])
    assert float(r["occlusion"][0][hit].min()) < 1.0


def test_files(env, tmp_path):
    from avatarcraft_amd import drivers
    from tests.test_mesh_export_host import read_ply
    from tests.test_texture_atlas_host import read_png
    net = env["net"]
    d = drivers.export_mesh(net, str(tmp_path / "a.obj"), bound=BOUND, resolution=24, texture_size=128, occlusion=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.mtl", "a.obj", "a.png", "a_ao.png"]
    mtl = (tmp_path / "a.mtl").read_text()
    assert "map_Kd a.png\n" in mtl and "map_Ka a_ao.png\n" in mtl
    ao = read_png(str(tmp_path / "a_ao.png"))
    assert ao.shape == (128, 128, 3) and all(np.array_equal(ao[..., k], d["occlusion_map"]) for k in range(3))
    assert np.array_equal(read_png(str(tmp_path / "a.png")), d["texture"])
    q = drivers.export_mesh(net, str(tmp_path / "a.ply"), bound=BOUND, resolution=24, occlusion=True)
    props, vert, _, _ = read_ply(str(tmp_path / "a.ply"))
    assert props[-1] == "float quality" and len(props) == 10 and np.array_equal(vert["quality"], q["occlusion"]) and q["occlusion"].dtype == np.float32
    assert np.array_equal(q["occlusion"], d["occlusion"])
    assert net.export_occlusion is None                                                # the driver put the switch back
    drivers.export_mesh(net, str(tmp_path / "b.ply"), bound=BOUND, resolution=24)
    assert len(read_ply(str(tmp_path / "b.ply"))[0]) == 9


def test_refusals_before_any_launch(env, pn, meshes):
    from avatarcraft_amd import _lib as L
    from avatarcraft_amd.mesh_occlusion import field_occlusion, mesh_bake_maps, occlusion_kit
    p, n = pn[0], pn[1]
    pos, tris = meshes[24]
    good = occlusion_kit(0.4)
    up = np.array([[0.0, 0.0, 1.0]], np.float32)
    bad = [dict(good, dirs=np.tile(up, (33, 1)), weights=np.full(33, 1.0 / 33, np.float32)),                  # K = 33
           dict(good, dirs=np.array([[np.sqrt(1 - 1e-4), 0.0, 0.01]], np.float32), weights=np.ones(1, np.float32)),      # lz = 0.01
           dict(good, dists=good["dists"][::-1].copy()), dict(good, gain=0.0)]
    for kit in bad:
        with pytest.raises(ValueError, match="occlusion_kit"):
            field_occlusion(env["gf"], p, n, BOUND, kit)
        with pytest.raises(ValueError, match="occlusion_kit"):
            mesh_bake_maps(env["gf"], pos, tris, 128, 8, BOUND, EPS, kit=kit)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        field_occlusion(env["gf"], p.cpu(), n, BOUND, good)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        field_occlusion(env["gf"], p, n.cpu(), BOUND, good)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        field_occlusion(env["gf"], p, n, BOUND, good, active=torch.ones(184, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="shape"):
        field_occlusion(env["gf"], p, n[:100].contiguous(), BOUND, good)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        mesh_bake_maps(env["gf"], pos.cpu(), tris, 128, 8, BOUND, EPS, kit=good)
    with pytest.raises(RuntimeError, match="cell 7 < 8"):
        mesh_bake_maps(env["gf"], pos, tris, 128, 7, BOUND, EPS, kit=good)
    bad_t = tris.clone(); bad_t[5, 1] = pos.shape[0]
    with pytest.raises(RuntimeError, match=r"outside \[0, 184\); nothing was launched"):
        mesh_bake_maps(env["gf"], pos, bad_t, 128, 8, BOUND, EPS, kit=good)
    # the raw entries: the same rules on the host, before any launch
    lib = L.lib()
    out = torch.full((184,), 7.0, device=DEV)
    def raw_kit(k):
        return L.ac_occlusion_opts(len(k["dirs"]), len(k["dists"]), k["dirs"].ctypes.data, k["weights"].ctypes.data, k["dists"].ctypes.data, k["gain"], k["level"])
    for kit in bad:
        kit = {k: (np.ascontiguousarray(v, np.float32) if isinstance(v, np.ndarray) else v) for k, v in kit.items()}
        rc = lib.ac_field_occlusion(C.byref(env["gf"].c), p.data_ptr(), n.data_ptr(), None, 184, BOUND, C.byref(raw_kit(kit)), out.data_ptr(), L.current_stream(DEV))
        assert rc == 1 and b"occlusion kit" in lib.ac_last_error()
    assert lib.ac_field_occlusion(C.byref(env["gf"].c), p.data_ptr(), n.data_ptr(), None, 184, 0.0, C.byref(raw_kit(good)), out.data_ptr(), L.current_stream(DEV)) == 1
    # occlusion given without a kit, and a kit without occlusion
    S = 128
    owner, o_img = torch.empty((S, S), dtype=torch.int32, device=DEV), torch.full((S, S), 7.0, device=DEV)
    atlas, opts = L.ac_atlas_opts(S, 8), L.ac_mesh_attr_opts(BOUND, EPS, 0.0, 0, TOL, cell(24))
    for bake_out, k in ((L.ac_bake_out(None, owner.data_ptr(), None, None, None, None, o_img.data_ptr()), None),
                        (L.ac_bake_out(None, owner.data_ptr(), None, None, None, None, None), C.byref(raw_kit(good)))):
        rc = lib.ac_mesh_bake_maps(C.byref(env["gf"].c), pos.data_ptr(), 184, tris.data_ptr(), tris.shape[0], C.byref(atlas), C.byref(opts), k, C.byref(bake_out),
                                   L.current_stream(DEV))
        assert rc == 1 and b"both or neither" in lib.ac_last_error()
    with pytest.raises(RuntimeError, match="both or neither"):
        L.check(1, "mesh_bake_maps")
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((o_img == 7).all())                         # nothing was written: nothing was launched
