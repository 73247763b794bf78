"""CPU tier of the mesh repair (ac_mesh_repair_count / _emit, csrc/mesh_repair.hip; avatarcraft_amd/mesh_repair.py; NeRFNetwork.export_manifold; manifold= of the
export drivers): the yardstick of the GPU tier (tests/mesh_repair_cases.py) against hand-worked meshes whose result is written out in literals and against the
counts its definition gave on the decimated, welded marching-cubes meshes of the CPU fixtures; the entries and their refusals, which come before any launch and so
run without a device; and the Python-level refusals and the model's switch.  The GPU tier (tests/test_gpu_mesh_repair.py) compares the kernels with the
yardstick, exactly."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_component_cases as MC
from tests import mesh_decimate_cases as K
from tests import mesh_repair_cases as R
from tests import mesh_weld_cases as W

NAMES = ("ac_mesh_repair_scratch", "ac_mesh_repair_count", "ac_mesh_repair_emit")


def _report(V, **kw):
    r = {**dict.fromkeys(R.REPORT_KEYS, 0), "vertices": V, "added": 0, **kw}
    r["vertices"] = V + r["added"]
    return r


def _after(r):
    return W.topology(r["triangles"], r["report"]["vertices"])


def _idempotent(P, r):
    again = R.repair(P[r["source"]], r["triangles"])
    assert again["report"]["added"] == 0 and np.array_equal(again["triangles"], r["triangles"])
    assert np.array_equal(again["source"], np.arange(r["report"]["vertices"]))


# ---------------------------------------------------------------------------------------------------- the yardstick, by hand
def test_two_tetrahedra_on_an_edge_come_apart_as_two_spheres():
    P, t = R.two_tetrahedra_on_an_edge()
    before = W.topology(t, 6)
    assert (before["nonmanifold"], before["boundary"], before["misoriented"], before["euler"]) == (1, 0, 0, 3)
    r = R.repair(P, t)
    assert r["report"] == _report(6, added=2, split=2, nonmanifold=1, paired=4)
    assert r["source"].tolist() == [0, 1, 2, 3, 4, 5, 0, 1] and r["source"].dtype == np.int32 and r["triangles"].dtype == np.int32
    assert np.array_equal(r["triangles"][:4], t[:4])                                       # the first body keeps the vertices: its fans hold the smallest corners
    assert np.array_equal(r["source"][r["triangles"]], t)                                  # the same triangles, order and orientation, under new names
    assert set(r["triangles"][4:].reshape(-1).tolist()) == {4, 5, 6, 7}
    after = _after(r)
    assert after["closed_manifold"] and after["euler"] == 4 and after["referenced"] == 8
    _idempotent(P, r)


def test_the_wedges_of_solid_are_paired_not_the_sheets_that_cross():
    """the same eight triangles with the second tetrahedron on the SAME side as the first would pair differently: here the two bodies lie on either side of the
    edge, and the pairs are (body one's two faces), (body two's two faces) -- whatever the ids say: under a permutation of the triangles it stays two spheres"""
    P, t = R.two_tetrahedra_on_an_edge()
    for seed in range(6):
        pt, p = W.permuted_triangles(t, seed=seed)
        r = R.repair(P, pt)
        after = _after(r)
        assert r["report"]["added"] == 2 and after["closed_manifold"] and after["euler"] == 4
        body = r["triangles"][np.argsort(p)]                                               # back in the original order
        assert len(set(body[:4].reshape(-1).tolist()) & set(body[4:].reshape(-1).tolist())) == 0


def test_two_tetrahedra_on_a_vertex_are_two_fans():
    P, t = R.two_tetrahedra_on_a_vertex()
    assert W.topology(t, 7)["closed_manifold"]                                             # the edge report cannot see it
    r = R.repair(P, t)
    assert r["report"] == _report(7, added=1, split=1) and r["source"].tolist() == [0, 1, 2, 3, 4, 5, 6, 0]
    assert np.array_equal(r["triangles"][:4], t[:4]) and np.array_equal(r["triangles"][4:], np.where(t[4:] == 0, 7, t[4:]))
    after = _after(r)
    assert after["closed_manifold"] and after["euler"] == 4
    _idempotent(P, r)


def test_a_fin_is_cut_off():
    P, t = R.fin()
    r = R.repair(P, t)
    assert r["report"] == _report(5, added=2, split=2, nonmanifold=1, paired=2, cut=1)
    assert np.array_equal(r["triangles"][:4], t[:4]) and r["triangles"][4].tolist() == [5, 6, 4] and r["source"].tolist() == [0, 1, 2, 3, 4, 0, 1]
    after = _after(r)
    assert (after["nonmanifold"], after["boundary"]) == (0, 3)
    _idempotent(P, r)


def test_an_edge_with_ten_uses_is_crowded():
    P, t = R.one_edge(10)
    r = R.repair(P, t)
    assert r["report"] == _report(12, added=18, split=2, nonmanifold=1, cut=10, crowded=1)  # ten fans at either end, one of them keeps the vertex
    assert _after(r)["boundary"] == 30
    P, t = R.one_edge(8, seed=1)                                                           # eight is not
    rep = R.repair(P, t)["report"]
    assert (rep["nonmanifold"], rep["crowded"], rep["paired"] + rep["cut"]) == (1, 0, 8)


def test_keys_that_tie_or_are_not_finite():
    P, t = R.fin()
    Q = P.copy()
    Q[4] = Q[2]                                                                            # the fin lies ON a face: equal keys, the use id decides
    r = R.repair(Q, t)
    assert (r["report"]["paired"], r["report"]["cut"], r["report"]["crowded"]) == (2, 1, 0)
    keys = R.use_keys(Q, 0, 1, [2, 4, 3])
    assert keys[0] == keys[1] and 0.0 <= min(keys) and max(keys) < 4.0
    Q = P.copy()
    Q[1] = Q[0]                                                                            # a zero-length edge: every key is 0
    assert R.use_keys(Q, 0, 1, [2, 3, 4]) == [0.0, 0.0, 0.0] and R.repair(Q, t)["report"]["crowded"] == 0
    Q = P.copy()
    Q[4] = np.nan                                                                          # a NaN position: treated as crowded
    r = R.repair(Q, t)
    assert (r["report"]["crowded"], r["report"]["cut"], r["report"]["paired"]) == (1, 3, 0)


def test_degenerate_and_out_of_range_triangles_are_counted_and_copied():
    P, t = R.two_tetrahedra_on_an_edge()
    mixed = np.concatenate([t[:3], [[0, 0, 1], [0, 1, 9], [-1, 2, 3]], t[3:]]).astype(np.int32)
    r = R.repair(P, mixed)
    assert r["report"]["invalid"] == 2 and r["report"]["degenerate"] == 1 and r["report"]["added"] == 2
    assert r["triangles"][3:6].tolist() == [[0, 0, 1], [0, 1, 9], [-1, 2, 3]]
    empty = R.repair(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert empty["report"] == _report(0) and empty["source"].shape == (0,) and empty["triangles"].shape == (0, 3)
    alone = R.repair(np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32))
    assert alone["report"] == _report(5) and alone["source"].tolist() == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------- decimated, welded marching-cubes meshes
@pytest.fixture(scope="module")
def shell_mesh(oracle):
    n = 32
    return oracle.marching_cubes(R.shell_volume(n), 0.0, den=n - 1.0, span=[2.0] * 3, lo=[-1.0] * 3)


# (vertices, triangles) after the weld; non-manifold edges before and after the repair; vertices added; uses paired; closed manifold afterwards
@pytest.mark.parametrize("k,size,nonmanifold,added,paired,closed", [(3, (214, 556), (82, 0), 132, 328, True), (2, (524, 1336), (144, 3), 174, 576, False)])
def test_the_thin_shell(shell_mesh, k, size, nonmanifold, added, paired, closed):
    from avatarcraft_amd.mesh_decimate import cluster_grid
    P, t = R.welded(*shell_mesh, cluster_grid(1.0, 32, k))
    assert (len(P), len(t)) == size and W.topology(t, len(P))["nonmanifold"] == nonmanifold[0]
    r = R.repair(P, t)
    rep, after = r["report"], _after(r)
    assert (rep["nonmanifold"], rep["added"], rep["paired"], rep["cut"], rep["crowded"]) == (nonmanifold[0], added, paired, 0, 0)
    assert (after["nonmanifold"], after["boundary"], after["misoriented"], after["closed_manifold"]) == (nonmanifold[1], 0, 0, closed)
    assert np.array_equal(r["source"][r["triangles"]], t) and np.array_equal(r["source"][:len(P)], np.arange(len(P)))
    _idempotent(P, r)


def test_the_noise_volume(oracle):
    padded, _ = MC.noise_volumes()
    v, t = oracle.marching_cubes(padded, 0.0)
    P, m = R.welded(v, t, K.grid_over(v.min(axis=0) - 1e-3, v.max(axis=0) + 1e-3, 2.0))
    assert (len(P), len(m)) == (3350, 13846) and W.topology(m, len(P))["nonmanifold"] == 3028
    r = R.repair(P, m)
    rep, after = r["report"], _after(r)
    assert (rep["nonmanifold"], rep["added"], rep["cut"], rep["crowded"], rep["paired"]) == (3028, 3167, 84, 0, 12336)
    assert (after["nonmanifold"], after["boundary"]) == (237, 76) and after["boundary"] <= rep["cut"]
    _idempotent(P, r)


def test_the_floater_meshes_come_back_unchanged(oracle):
    from avatarcraft_amd.mesh_decimate import cluster_grid
    n = 40
    v, t = oracle.marching_cubes(MC.body_with_floaters(n), 0.0, den=n - 1.0, span=[2.0] * 3, lo=[-1.0] * 3)
    for k in (2, 3, 5):
        P, m = R.welded(v, t, cluster_grid(1.0, n, k))
        r = R.repair(P, m)
        assert r["report"] == _report(len(P)) and np.array_equal(r["triangles"], m) and r["triangles"].dtype == m.dtype


# ---------------------------------------------------------------------------------------------------- the C entries, without a device
def test_the_entries_are_declared_and_bound():
    from avatarcraft_amd import _lib, build
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avatarcraft_hip.h")).read()
    for name, ret, arity in zip(NAMES, ("size_t", "int", "int"), (2, 8, 10)):
        assert name in _lib.EXPORTS and re.search(r"\b%s %s\s*\(" % (ret, name), hdr)
        assert len(_lib._SIGS[name][0]) == arity
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == arity         # the header's parameter list and the binding's agree
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().ac_version() == 10 and "mesh_repair.hip" in build.SOURCES             # added entries, no struct changed
    src = lambda f: open(os.path.join(os.path.dirname(_lib.__file__), "csrc", f)).read()
    assert "cc_unite" in src("mesh_index.hpp") and "mi::cc_unite" in src("mesh_components.hip") and "mi::cc_unite" in src("mesh_repair.hip")
    assert "void cc_unite" not in src("mesh_components.hip") and "void cc_unite" not in src("mesh_repair.hip")      # one copy of the union-find


def test_the_scratch_size_is_a_host_function():
    from avatarcraft_amd import _lib
    sc = _lib.lib().ac_mesh_repair_scratch
    assert sc(2 ** 31, 0) == 0 and sc(0, 2 ** 31) == 0 and sc(10, (2 ** 31 - 1) // 3 + 1) == 0   # indices and corner ids are int32
    V, T = 400_000, 790_000                                                                # the 2048^3 export at decimate = 2
    cap = 1 << int(np.ceil(np.log2(6 * T)))
    assert 24 * cap + 36 * T + 8 * V <= sc(V, T) < 24 * cap + 37 * T + 9 * V
    assert sc(10, 2000) >= sc(10, 1000) and sc(1025, 10) >= sc(1000, 10) and sc(0, 0) >= 0


def refusals():
    """every AC_ERR_BAD_ARG rule of the two entries: (entry, changed arguments, what the message says).  The addresses are never read."""
    shared = [(dict(tris=None), "NULL buffer"), (dict(verts=None), "NULL buffer"), (dict(scratch=None), "NULL buffer"), (dict(V=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"),
              (dict(T=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"), (dict(T=2 ** 30, nbytes=2 ** 44), r"3 T = 3 x 1073741824 above 2\^31 - 1 \(corner ids"),
              (dict(V=0), "2000 triangles over no vertex"), (dict(short=1), "scratch of %d bytes needed, %d given")]
    out = [(e, kw, m) for e in ("repair_count", "repair_emit") for kw, m in shared]
    out += [("repair_count", dict(counts=None), "NULL counts")]
    out += [("repair_emit", dict(nv=999), r"n_vertices 999 outside \[V, V \+ 3 T\] = \[1000, 7000\]"), ("repair_emit", dict(nv=7001), "n_vertices 7001 outside")]
    out += [("repair_emit", {k: None}, "NULL output") for k in ("tris_out", "source")]
    return out


def check_refusals():
    """each rule comes back as AC_ERR_BAD_ARG (1) with its message, before a buffer is touched or anything is launched"""
    from avatarcraft_amd import _lib
    lib = _lib.lib()
    P = 4096                                                     # a non-NULL address that nothing dereferences
    V, T = 1000, 2000
    need = lib.ac_mesh_repair_scratch(V, T)

    def call(entry, verts=P, tris=P, T=T, V=V, scratch=P, nbytes=None, short=0, counts=P, tris_out=P, source=P, nv=1010):
        head = (verts, tris, T, V, scratch, (need if nbytes is None else nbytes) - short)
        if entry == "repair_count":
            return lib.ac_mesh_repair_count(*head, counts, None)
        return lib.ac_mesh_repair_emit(*head, tris_out, source, nv, None)
    for entry, kw, match in refusals():
        assert call(entry, **kw) == 1, (entry, kw)
        err = lib.ac_last_error().decode()
        if "%d" in match:
            match = match % (need, need - 1)
        assert re.search(match, err) and "mesh_" + entry in err, (entry, kw, err)
    return len(refusals())


def test_every_entry_refuses_before_any_launch():
    assert check_refusals() == 21


# ---------------------------------------------------------------------------------------------------- Python and the model
def test_python_refuses_before_anything_is_computed():
    from avatarcraft_amd import mesh_repair
    assert mesh_repair.REPORT_KEYS == R.REPORT_KEYS
    v, t = torch.zeros((5, 3), dtype=torch.float32), torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="vertices must be a CUDA tensor \\(there is no CPU path\\)"):
        mesh_repair.mesh_repair(v, t)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh_repair.mesh_repair(v.numpy(), t.numpy())
    with pytest.raises(RuntimeError, match="textured mesh"):
        mesh_repair.repair_mesh(dict(vertices=v, triangles=t, uv=np.zeros((4, 3, 2))))
    with pytest.raises(RuntimeError, match="textured mesh"):
        mesh_repair.repair_mesh(dict(vertices=v, triangles=t, texture=np.zeros((8, 8, 3), np.uint8)))
    with pytest.raises(RuntimeError, match="CUDA tensors \\(there is no CPU path\\)"):
        mesh_repair.repair_mesh(dict(vertices=v, triangles=t))
    with pytest.raises(RuntimeError, match="CUDA tensors \\(there is no CPU path\\)"):
        mesh_repair.repair_mesh(dict(vertices=v.numpy(), triangles=t.numpy(), normals=np.zeros((5, 3), np.float32)))


def test_the_model_switch():
    from avatarcraft_amd import drivers
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    from tests.test_instant_nsr_package_host import SIGNATURES
    assert inspect.getattr_static(NeRFNetwork, "export_manifold") is False
    for name in ("extract_geometry", "extract_colored_mesh", "extract_textured_mesh"):
        assert str(inspect.signature(inspect.getattr_static(NeRFNetwork, name))) == SIGNATURES[name]      # frozen: the way in is the switch
    torch.manual_seed(0)
    net = NeRFNetwork()                                                                # on the CPU
    net.export_manifold = True
    with pytest.raises(RuntimeError, match="export_manifold"):
        net.extract_geometry(1.6, 12)                                                  # the native mesher only: not the CPU's fall-back mesher
    with pytest.raises(RuntimeError, match="export_manifold"):
        net.extract_geometry(1.6, 12, mesher="tetra")
    for call in (lambda: net.extract_colored_mesh(1.6, 12), lambda: net.extract_textured_mesh(1.6, 12, texture_size=64)):
        with pytest.raises(RuntimeError, match="on the GPU"):
            call()
    del net.export_manifold
    assert net.export_manifold is False
    seen = []

    def boom(*a, **kw):
        seen.append((net.export_manifold, net.export_weld, kw))
        raise ZeroDivisionError("after the switch was set")
    net.extract_colored_mesh = net.extract_textured_mesh = boom
    for path in ("never_written.ply", "never_written.obj"):
        with pytest.raises(ZeroDivisionError):
            drivers.export_mesh(net, path, resolution=12, manifold=True, decimate=2)
        assert net.export_manifold is False and net.export_weld is False               # restored after the exception
        with pytest.raises(ZeroDivisionError):
            drivers.export_mesh(net, path, resolution=12, weld=True, manifold=True, decimate=2)
        assert net.export_manifold is False and net.export_weld is False
    assert [s[:2] for s in seen] == [(True, False), (True, True)] * 2 and all(s[2] == dict(decimate=2) for s in seen)
    assert "manifold" in drivers.export_mesh.__doc__ and "manifold" in drivers.export_animation.__doc__
