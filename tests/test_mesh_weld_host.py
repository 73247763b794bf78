"""CPU tier of the mesh weld and the topology report (ac_mesh_weld_count / _emit, ac_mesh_topology, csrc/mesh_weld.hip; avatarcraft_amd/mesh_weld.py;
NeRFNetwork.export_weld; weld= of the export drivers): the yardstick of the GPU tier (tests/mesh_weld_cases.py) against hand-worked index buffers whose result is
written out in literals; what the weld does to the decimated marching-cubes mesh of tests/test_mesh_decimate_host.py, where vertex clustering leaves back-to-back
pairs; the entries and their refusals, which come before any launch and so run without a device; and the Python-level refusals and the model's switch.  The GPU
tier (tests/test_gpu_mesh_weld.py) compares the kernels with the yardstick, exactly."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_component_cases as MC
from tests import mesh_decimate_cases as K
from tests import mesh_weld_cases as W

NAMES = ("ac_mesh_weld_scratch", "ac_mesh_weld_count", "ac_mesh_weld_emit", "ac_mesh_topology_scratch", "ac_mesh_topology")


def _report(**kw):
    return {**dict.fromkeys(W.REPORT_KEYS, 0), **kw}


# ---------------------------------------------------------------------------------------------------- the yardstick, by hand
def test_a_back_to_back_pair_cancels():
    r = W.weld([[0, 1, 2], [2, 1, 0]], 3)
    assert r["report"] == _report(cancelled=2) and r["triangles"].shape == (0, 3) and r["kept_triangles"].shape == (0,)
    assert r["vertex_map"].tolist() == [-1, -1, -1] and r["kept_vertices"].shape == (0,)
    for k in ("vertex_map", "kept_vertices", "triangles", "kept_triangles"):
        assert r[k].dtype == np.int32


def test_a_repeated_triangle_is_kept_once_and_orphans_go():
    r = W.weld([[0, 1, 2], [1, 2, 0], [4, 5, 6]], 7)
    assert r["kept_triangles"].tolist() == [0, 2] and r["report"] == _report(vertices=6, triangles=2, repeated=1, excess=1)
    assert r["vertex_map"].tolist() == [0, 1, 2, -1, 3, 4, 5] and r["kept_vertices"].tolist() == [0, 1, 2, 4, 5, 6]
    assert r["triangles"].tolist() == [[0, 1, 2], [3, 4, 5]]


def test_the_majority_sign_keeps_its_first_member_in_its_own_corner_order():
    t = [[5, 7, 9], [9, 7, 5], [7, 5, 9], [5, 9, 7]]                                      # +, -, -, -: net = -2
    assert W.signs(np.array(t)).tolist() == [True, False, False, False]
    r = W.weld(t, 10)
    assert r["kept_triangles"].tolist() == [1] and r["triangles"].tolist() == [[2, 1, 0]]  # the first - member, as it stands (not rotated, not sorted)
    assert r["report"] == _report(vertices=3, triangles=1, repeated=3, excess=1)
    r = W.weld(t[:3] + [[5, 7, 9], [9, 5, 7]], 10)                                         # +, -, -, +, +: net = +1 -> triangle 0
    assert r["kept_triangles"].tolist() == [0] and r["report"] == _report(vertices=3, triangles=1, repeated=4, excess=0)


def test_degenerate_and_out_of_range_triangles_are_counted():
    t = [[0, 1, 2], [1, 1, 2], [0, 3, 0], [0, 1, 4], [-1, 1, 2], [2, 2, 2], [2, 3, 1]]
    r = W.weld(t, 4)
    assert r["report"] == _report(vertices=4, triangles=2, invalid=2, degenerate=3) and r["kept_triangles"].tolist() == [0, 6]
    top = W.topology(t, 4)
    assert (top["faces"], top["invalid"], top["degenerate"], top["referenced"], top["edges"]) == (2, 2, 3, 4, 5)
    assert W.topology([[4, 4, 4]], 4)["invalid"] == 1                                     # out of range comes before degenerate
    empty = W.weld(np.zeros((0, 3), np.int32), 0)
    assert empty["report"] == _report() and empty["vertex_map"].shape == (0,) and W.topology(np.zeros((0, 3)), 5)["euler"] == 0


def test_topology_of_tetrahedra():
    top = W.topology(W.TETRAHEDRON, 4)
    assert top == dict(edges=6, boundary=0, nonmanifold=0, misoriented=0, referenced=4, faces=4, invalid=0, degenerate=0, euler=2, closed_manifold=True)
    MC.mesh_checks(np.zeros((4, 3)), np.array(W.TETRAHEDRON))                              # (closed and consistently oriented by the project's own check)
    top = W.topology(W.TETRAHEDRON[:3], 4)
    assert (top["edges"], top["boundary"], top["nonmanifold"], top["misoriented"], top["closed_manifold"]) == (6, 3, 0, 0, False)
    two = W.TETRAHEDRON + np.array([0, 1, 4, 5])[np.array(W.TETRAHEDRON)].tolist()           # a second one on the edge (0, 1)
    top = W.topology(two, 6)
    assert (top["edges"], top["boundary"], top["nonmanifold"], top["misoriented"], top["referenced"], top["faces"]) == (11, 0, 1, 0, 6, 8)
    flipped = [W.TETRAHEDRON[0][::-1]] + W.TETRAHEDRON[1:]
    top = W.topology(flipped, 4)
    assert (top["edges"], top["boundary"], top["nonmanifold"], top["misoriented"], top["closed_manifold"]) == (6, 0, 0, 3, False)
    assert W.weld(W.TETRAHEDRON, 4)["report"] == _report(vertices=4, triangles=4)           # nothing to weld: everything stays
    t, V = W.low_word_twins()
    top = W.topology(t, V)
    assert (top["edges"], top["referenced"], top["faces"]) == (9, 5, 8)                     # (6 if edges were told apart by the low word of their key)


# ---------------------------------------------------------------------------------------------------- the decimated floater mesh
@pytest.fixture(scope="module")
def floater_mesh(oracle):
    n = 40
    v, t = oracle.marching_cubes(MC.body_with_floaters(n), 0.0, den=n - 1.0, span=[2.0] * 3, lo=[-1.0] * 3)
    MC.mesh_checks(v, t)
    return v, t


# (clusters, triangles) before and after the weld; the pairs K.duplicate_triangles finds before it; non-manifold edges before it
@pytest.mark.parametrize("k,before,after,pairs,nonmanifold", [(1, (1510, 3004), (1510, 3004), 0, 0), (2, (450, 884), (448, 884), 0, 0),
                                                             (3, (219, 422), (215, 418), 2, 2), (5, (92, 168), (88, 164), 2, 1)])
def test_the_weld_on_the_decimated_floater_mesh(floater_mesh, k, before, after, pairs, nonmanifold):
    from avatarcraft_amd.mesh_decimate import cluster_grid
    v, t = floater_mesh
    c = K.cluster(v, t, cluster_grid(1.0, 40, k))
    V, m = len(c["leader"]), c["triangles"]
    assert (V, len(m)) == before and K.duplicate_triangles(m) == (0, pairs)
    w = W.weld(m, V)
    rep = w["report"]
    assert rep == _report(vertices=after[0], triangles=after[1], cancelled=2 * pairs)      # what the definitions' prototype gave
    assert K.duplicate_triangles(w["triangles"]) == (0, 0)
    assert rep["excess"] == 0                                                              # the premise of the edge balance: asserted, so that it is not vacuous
    fwd, fc, rev, rc = K.edge_balance(w["triangles"])
    assert np.array_equal(fwd, rev) and np.array_equal(fc, rc)
    # bookkeeping: survivors in order, re-indexed through the map; a kept vertex is one that a survivor names
    assert (np.diff(w["kept_triangles"]) > 0).all() and np.array_equal(w["triangles"], w["vertex_map"][m[w["kept_triangles"]]])
    assert np.array_equal(np.flatnonzero(w["vertex_map"] >= 0), w["kept_vertices"]) and np.array_equal(w["vertex_map"][w["kept_vertices"]], np.arange(after[0]))
    assert np.array_equal(np.unique(m[w["kept_triangles"]]), w["kept_vertices"])
    top_before, top_after = W.topology(m, V), W.topology(w["triangles"], after[0])
    assert top_before["nonmanifold"] == nonmanifold and top_before["closed_manifold"] == (pairs == 0)
    assert top_before["referenced"] == V - {1: 0, 2: 2, 3: 2, 5: 0}[k]                      # orphans there before any weld: clusters whose triangles all collapsed
    assert top_after["closed_manifold"] and top_after["referenced"] == after[0] and top_after["faces"] == after[1]
    assert top_after["edges"] == {1: 4506, 2: 1326, 3: 627, 5: 246}[k] and 2 * top_after["edges"] == 3 * top_after["faces"]
    if pairs == 0:
        assert np.array_equal(w["kept_triangles"], np.arange(len(m)))                      # nothing but orphan vertices changes


# ---------------------------------------------------------------------------------------------------- the C entries, without a device
def test_the_entries_are_declared_and_bound():
    from avatarcraft_amd import _lib, build
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avatarcraft_hip.h")).read()
    for name, ret, arity in zip(NAMES, ("size_t", "int", "int", "size_t", "int"), (2, 7, 12, 2, 7)):
        assert name in _lib.EXPORTS and re.search(r"\b%s %s\s*\(" % (ret, name), hdr)
        assert len(_lib._SIGS[name][0]) == arity
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == arity         # the header's parameter list and the binding's agree
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().ac_version() == 10 and "mesh_weld.hip" in build.SOURCES               # added entries, no struct changed
    src = lambda f: open(os.path.join(os.path.dirname(_lib.__file__), "csrc", f)).read()
    assert "key_slot" in src("mesh_index.hpp") and "mi::key_slot" in src("mesh_cluster.hip") and "mi::key_slot" in src("mesh_weld.hip")
    assert "mcl_slot" not in src("mesh_cluster.hip")                                        # one copy of the 64-bit key claim


def test_scratch_sizes_are_host_functions():
    from avatarcraft_amd import _lib
    for sc, per_slot, slots_per_tri in ((_lib.lib().ac_mesh_weld_scratch, 20, 2), (_lib.lib().ac_mesh_topology_scratch, 16, 6)):
        assert sc(2 ** 31, 0) == 0 and sc(0, 2 ** 31) == 0                                  # indices are int32
        V, T = 400_000, 790_000                                                            # the 2048^3 export at decimate = 2
        cap = 1 << int(np.ceil(np.log2(slots_per_tri * T)))
        assert per_slot * cap + V <= sc(V, T) < per_slot * cap + V + 8 * T
        assert sc(2 ** 31 - 1, 2 ** 31 - 1) > per_slot * 2 ** 32 and sc(0, 0) >= 0
        assert sc(10, 2000) >= sc(10, 1000) and sc(1025, 10) >= sc(1000, 10)


def refusals():
    """every AC_ERR_BAD_ARG rule of the three entries: (entry, changed arguments, what the message says).  The addresses are never read."""
    shared = [(dict(tris=None), "NULL buffer"), (dict(scratch=None), "NULL buffer"), (dict(V=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"),
              (dict(T=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"), (dict(V=0), "2000 triangles over no vertex"), (dict(short=1), "scratch of %d bytes needed, %d given")]
    out = [(e, kw, m) for e in ("weld_count", "weld_emit", "topology") for kw, m in shared]
    out += [("weld_count", dict(counts=None), "NULL counts"), ("topology", dict(counts=None), "NULL counts")]
    out += [("weld_emit", dict(nv=1001), "n_kept_vertices 1001 > V 1000"), ("weld_emit", dict(nt=2001), "n_kept_triangles 2001 > T 2000")]
    out += [("weld_emit", {k: None}, "NULL output") for k in ("vmap", "kept_v", "tris_out", "kept_t")]
    return out


def check_refusals():
    """each rule comes back as AC_ERR_BAD_ARG (1) with its message, before a buffer is touched or anything is launched"""
    from avatarcraft_amd import _lib
    lib = _lib.lib()
    P = 4096                                                     # a non-NULL address that nothing dereferences
    V, T = 1000, 2000
    need = dict(weld_count=lib.ac_mesh_weld_scratch(V, T), topology=lib.ac_mesh_topology_scratch(V, T))
    need["weld_emit"] = need["weld_count"]

    def call(entry, tris=P, T=T, V=V, scratch=P, nbytes=None, short=0, counts=P, vmap=P, kept_v=P, nv=10, tris_out=P, kept_t=P, nt=10):
        head = (tris, T, V, scratch, (need[entry] if nbytes is None else nbytes) - short)
        if entry == "weld_count":
            return lib.ac_mesh_weld_count(*head, counts, None)
        if entry == "topology":
            return lib.ac_mesh_topology(*head, counts, None)
        return lib.ac_mesh_weld_emit(*head, vmap, kept_v, nv, tris_out, kept_t, nt, None)
    for entry, kw, match in refusals():
        assert call(entry, **kw) == 1, (entry, kw)
        err = lib.ac_last_error().decode()
        if "%d" in match:
            match = match % (need[entry], need[entry] - 1)
        assert re.search(match, err) and "mesh_" + entry in err, (entry, kw, err)
    return len(refusals())


def test_every_entry_refuses_before_any_launch():
    assert check_refusals() == 26


# ---------------------------------------------------------------------------------------------------- Python and the model
def test_python_refuses_before_anything_is_computed():
    from avatarcraft_amd import mesh_weld
    v, t = torch.zeros((5, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int32)
    for fn in (mesh_weld.mesh_weld, mesh_weld.mesh_topology):
        with pytest.raises(RuntimeError, match="triangles must be a CUDA tensor \\(there is no CPU path\\)"):
            fn(t, 5)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(t.numpy(), 5)
    with pytest.raises(RuntimeError, match="textured mesh"):
        mesh_weld.weld_mesh(dict(vertices=v, triangles=t, uv=np.zeros((4, 3, 2))))
    with pytest.raises(RuntimeError, match="textured mesh"):
        mesh_weld.weld_mesh(dict(vertices=v, triangles=t, texture=np.zeros((8, 8, 3), np.uint8)))
    with pytest.raises(RuntimeError, match="CUDA tensors \\(there is no CPU path\\)"):
        mesh_weld.weld_mesh(dict(vertices=v, triangles=t))
    with pytest.raises(RuntimeError, match="CUDA tensors \\(there is no CPU path\\)"):
        mesh_weld.weld_mesh(dict(vertices=v.numpy(), triangles=t.numpy(), normals=np.zeros((5, 3), np.float32)))


def test_the_model_switch():
    from avatarcraft_amd import drivers
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    from tests.test_instant_nsr_package_host import SIGNATURES
    assert inspect.getattr_static(NeRFNetwork, "export_weld") is False
    for name in ("extract_geometry", "extract_colored_mesh", "extract_textured_mesh"):
        assert str(inspect.signature(inspect.getattr_static(NeRFNetwork, name))) == SIGNATURES[name]      # frozen: the way in is the switch
        assert list(inspect.signature(getattr(NeRFNetwork, name)).parameters)[-1] == "decimate"
    torch.manual_seed(0)
    net = NeRFNetwork()                                                                # on the CPU
    net.export_weld = True
    with pytest.raises(RuntimeError, match="export_weld"):
        net.extract_geometry(1.6, 12)                                                  # the native mesher only: not the CPU's fall-back mesher
    with pytest.raises(RuntimeError, match="export_weld"):
        net.extract_geometry(1.6, 12, mesher="tetra")
    for call in (lambda: net.extract_colored_mesh(1.6, 12), lambda: net.extract_textured_mesh(1.6, 12, texture_size=64)):
        with pytest.raises(RuntimeError, match="on the GPU"):
            call()
    del net.export_weld
    assert net.export_weld is False
    seen = []

    def boom(*a, **kw):
        seen.append((net.export_weld, kw))
        raise ZeroDivisionError("after the switch was set")
    net.extract_colored_mesh = net.extract_textured_mesh = boom
    for path in ("never_written.ply", "never_written.obj"):
        with pytest.raises(ZeroDivisionError):
            drivers.export_mesh(net, path, resolution=12, weld=True, decimate=2)
        assert net.export_weld is False                                                # restored after the exception
    assert len(seen) == 2 and seen[0] == (True, dict(decimate=2)) and all(s[0] is True and "weld" not in s[1] for s in seen) and net.export_weld is False
    assert "weld" in drivers.export_mesh.__doc__ and "weld" in drivers.export_animation.__doc__
