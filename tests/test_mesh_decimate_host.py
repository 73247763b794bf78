"""CPU tier of the mesh decimation (ac_mesh_cluster_count / _emit, csrc/mesh_cluster.hip; avatarcraft_amd/mesh_decimate.py; decimate= of the model's extractors):
the yardstick of the GPU tier (tests/mesh_decimate_cases.py) against hand-worked meshes whose result is written out in literals; cluster_grid and its refusals;
the invariants of vertex clustering on the oracle's marching-cubes mesh; the entries and their refusals, which come before any launch and so run without a device;
and the Python-level refusals, which come before anything is computed.  The GPU tier (tests/test_gpu_mesh_decimate.py) compares the kernels with the yardstick,
exactly."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_component_cases as MC
from tests import mesh_decimate_cases as K

NAMES = ("ac_mesh_cluster_scratch", "ac_mesh_cluster_count", "ac_mesh_cluster_emit")


# ---------------------------------------------------------------------------------------------------- the yardstick, by hand
def test_two_triangles_sharing_a_cell():
    """a 2^3 grid of unit cells; vertices 0 and 1 share cell (0, 0, 0), the others have cells of their own"""
    v = [[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]]
    t = [[0, 1, 2], [0, 2, 3], [1, 4, 2]]
    r = K.cluster(v, t, K.grid(0.0, 1.0, 2))
    assert r["cluster"].tolist() == [0, 0, 1, 2, 3] and r["leader"].tolist() == [0, 2, 3, 4] and r["members"].tolist() == [2, 1, 1, 1]
    assert r["positions"].tolist() == [[0.5, 0.25, 0.25], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5]]
    assert r["triangles"].tolist() == [[0, 1, 2], [0, 3, 1]] and r["kept_triangles"].tolist() == [1, 2]      # (0, 1, 2) collapsed: two corners in one cluster
    assert r["bad_vertices"] == 0 and r["bad_triangles"] == 0
    # the ids reversed: the leader of the shared cell is now vertex 3 (old 1), clusters are numbered by ascending leader, orientation is kept
    r = K.cluster(v[::-1], 4 - np.array(t), K.grid(0.0, 1.0, 2))
    assert r["cluster"].tolist() == [0, 1, 2, 3, 3] and r["leader"].tolist() == [0, 1, 2, 3] and r["members"].tolist() == [1, 1, 1, 2]
    assert r["positions"][3].tolist() == [0.5, 0.25, 0.25] and r["triangles"].tolist() == [[3, 2, 1], [3, 0, 2]]
    for dt in ("cluster", "leader", "members", "triangles", "kept_triangles"):
        assert r[dt].dtype == np.int32
    assert r["positions"].dtype == np.float64


def test_a_vertex_on_a_cell_face_belongs_to_the_upper_cell():
    g = K.grid(0.0, 1.0, 2)
    valid, cell, q, key = K.cells([[1.0, 0.5, 0.5]], g)
    assert valid.tolist() == [True] and cell.tolist() == [[1, 0, 0]] and q.tolist() == [[0, 2 ** 29, 2 ** 29]] and key.tolist() == [4]
    r = K.cluster([[1.0, 0.5, 0.5], [0.999999, 0.5, 0.5]], [[0, 1, 1]], g)
    assert r["cluster"].tolist() == [0, 1] and r["positions"][0].tolist() == [1.0, 0.5, 0.5] and r["triangles"].shape == (0, 3)
    valid, cell, q, key = K.cells([[0.0, -0.5, 1.0]], K.grid([-1.0, -1.0, -1.0], 0.5, [4, 5, 6]))
    assert cell.tolist() == [[2, 1, 4]] and q.tolist() == [[0, 0, 0]] and key.tolist() == [(2 * 5 + 1) * 6 + 4]


def test_a_vertex_at_the_upper_bound_is_kept_by_the_slack_and_clamped():
    from avatarcraft_amd.mesh_decimate import cluster_grid
    g = cluster_grid(1.6, 5, 2)                                                        # four marching-cubes cells, two cluster cells per axis
    b = float(np.float32(1.6))
    assert g == dict(lo=[-b] * 3, h=2 * (2 * b) / 4, n=[2] * 3) and g["h"] == b
    valid, cell, q, key = K.cells([[b, b, b], [b, -b, 0.0]], g)                         # t = 2 = n: valid by the slack of one cell, in the LAST cell with f = 1
    assert valid.tolist() == [True, True] and cell.tolist() == [[1, 1, 1], [1, 0, 1]] and q.tolist() == [[2 ** 30] * 3, [2 ** 30, 0, 0]]
    r = K.cluster([[b, b, b]], np.zeros((0, 3), np.int32), g)
    assert r["positions"].tolist() == [[b, b, b]] and r["members"].tolist() == [1]
    # what is not in the grid: beyond the slack, below the lower corner, not finite -- and the triangles that name them or an index outside [0, V)
    v = [[-1.0, -1.0, -1.0], [b + g["h"], 0.0, 0.0], [-b - 1e-9, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1.0, 1.0, 1.0], [-1.0, 1.0, 1.0]]
    t = [[0, 6, 7], [0, 1, 6], [0, 6, 8], [-1, 0, 6], [7, 6, 0], [3, 3, 3]]
    r = K.cluster(v, t, g)
    assert r["bad_vertices"] == 5 and r["bad_triangles"] == 4 and r["cluster"].tolist() == [0, -1, -1, -1, -1, -1, 1, 2]
    assert r["leader"].tolist() == [0, 6, 7] and r["triangles"].tolist() == [[0, 1, 2], [2, 1, 0]] and r["kept_triangles"].tolist() == [0, 4]
    assert K.duplicate_triangles(r["triangles"]) == (0, 1) and K.duplicate_triangles([[0, 1, 2], [1, 2, 0], [4, 5, 6]]) == (1, 0)


def test_cluster_grid_and_its_refusals():
    from avatarcraft_amd.mesh_decimate import cluster_grid
    b = float(np.float32(1.6))
    g = cluster_grid(1.6, 512, 2)
    assert g["lo"] == [-b] * 3 and g["n"] == [256] * 3 and g["h"] == 2.0 * (2 * b) / 511
    assert cluster_grid(1.6, 512, 1)["n"] == [511] * 3 and cluster_grid(1.6, 512, 1.5)["n"] == [341] * 3 and cluster_grid(1.6, 512, 4)["n"] == [128] * 3
    assert cluster_grid(1.6, 512, 1000)["n"] == [1] * 3 and cluster_grid(1.0, 40, np.float32(3))["h"] == 3.0 * 2.0 / 39
    assert cluster_grid(1.6, 2 ** 21 + 1, 1)["n"] == [2 ** 21] * 3
    for k in (0, 0.99, -2, float("nan"), float("inf"), True, "2", None, [2]):
        with pytest.raises(ValueError, match="cluster_grid: k"):
            cluster_grid(1.6, 512, k)
    with pytest.raises(ValueError, match="more than 2\\^21"):
        cluster_grid(1.6, 2 ** 21 + 2, 1)
    for res in (1, 0, 2.5, True, "512"):
        with pytest.raises(ValueError, match="cluster_grid: resolution"):
            cluster_grid(1.6, res, 2)
    for bound in (0.0, -1.0, float("nan"), float("inf"), "wide"):
        with pytest.raises(ValueError, match="cluster_grid: bound"):
            cluster_grid(bound, 512, 2)


# ---------------------------------------------------------------------------------------------------- invariants on a marching-cubes mesh
@pytest.fixture(scope="module")
def floater_mesh(oracle):
    n = 40
    v, t = oracle.marching_cubes(MC.body_with_floaters(n), 0.0, den=n - 1.0, span=[2.0] * 3, lo=[-1.0] * 3)
    MC.mesh_checks(v, t)                                                               # closed and consistently oriented: what the edge balance rests on
    assert (len(v), len(t)) == (2096, 4176)
    return v, t


@pytest.mark.parametrize("k,counts", [(1, None), (1.5, (694, 1372)), (2, (450, 884)), (3, None), (4, (138, 260))])
def test_edge_balance_and_bookkeeping_on_the_floater_mesh(floater_mesh, k, counts):
    """dropping only collapsed triangles from a closed oriented mesh leaves every directed edge u -> v as often as v -> u.  Strict manifoldness is NOT asserted: it
    fails at k = 3, where a thin sheet collapses into back-to-back pairs.  counts: what the prototype of the definitions gave."""
    from avatarcraft_amd.mesh_decimate import cluster_grid
    v, t = floater_mesh
    r = K.cluster(v, t, cluster_grid(1.0, 40, k))
    assert r["bad_vertices"] == 0 and r["bad_triangles"] == 0
    nc, nt = len(r["leader"]), len(r["triangles"])
    if counts is not None:
        assert (nc, nt) == counts
    assert 0 < nc < len(v) and 0 < nt < len(t)
    fwd, fc, rev, rc = K.edge_balance(r["triangles"])
    assert np.array_equal(fwd, rev) and np.array_equal(fc, rc)
    # bookkeeping: V' + removed = V; every cluster has its leader as its smallest member; surviving triangles name three different clusters, in order
    assert r["members"].sum() == len(v) and nc + int((r["members"] - 1).sum()) == len(v) and r["members"].min() >= 1
    assert (np.diff(r["leader"]) > 0).all() and np.array_equal(r["cluster"][r["leader"]], np.arange(nc))
    first = np.full(nc, len(v))
    np.minimum.at(first, r["cluster"], np.arange(len(v)))
    assert np.array_equal(first, r["leader"])
    m = r["triangles"]
    assert (m[:, 0] != m[:, 1]).all() and (m[:, 1] != m[:, 2]).all() and (m[:, 0] != m[:, 2]).all() and (np.diff(r["kept_triangles"]) > 0).all()
    assert np.array_equal(m, r["cluster"][t[r["kept_triangles"]]])
    g = cluster_grid(1.0, 40, k)
    assert np.abs(r["positions"] - v[r["leader"]]).max() <= g["h"]                     # the mean lies in the leader's cell
    if k == 3:
        assert K.duplicate_triangles(m)[1] > 0                                         # the back-to-back pairs the header speaks of: kept


# ---------------------------------------------------------------------------------------------------- the C entries, without a device
def test_the_entries_are_declared_and_bound():
    from avatarcraft_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avatarcraft_hip.h")).read()
    for name, ret, arity in zip(NAMES, ("size_t", "int", "int"), (2, 10, 15)):
        assert name in _lib.EXPORTS and re.search(r"\b%s %s\s*\(" % (ret, name), hdr)
        assert len(_lib._SIGS[name][0]) == arity
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == arity      # the header's parameter list and the binding's agree
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().ac_version() == 10                                                # added entries, no struct of an existing call changed
    import ctypes
    assert ctypes.sizeof(_lib.ac_cluster_grid) == 48 and _lib.ac_cluster_grid.h.offset == 24 and _lib.ac_cluster_grid.n.offset == 32


def test_scratch_size_is_a_host_function():
    from avatarcraft_amd import _lib
    sc = _lib.lib().ac_mesh_cluster_scratch
    assert sc(2 ** 31, 0) == 0 and sc(0, 2 ** 31) == 0                                  # indices are int32
    V, T = 1_580_000, 3_160_000                                                         # the 2048^3 streamed export: a table of 2^22 slots
    assert 44 * 2 ** 22 + 8 * V <= sc(V, T) < 44 * 2 ** 22 + 8 * V + 0.02 * 12 * T
    assert sc(2 ** 31 - 1, 2 ** 31 - 1) > 44 * 2 ** 32 and sc(0, 0) >= 0
    assert sc(1000, 10) <= sc(1025, 10) and sc(10, 2000) >= sc(10, 1000)


def refusals():
    """every AC_ERR_BAD_ARG rule of the two entries: (entry, changed arguments, what the message says).  The addresses are never read."""
    both = [(dict(verts=None), "NULL"), (dict(tris=None), "NULL"), (dict(scratch=None), "NULL"), (dict(grid=None), "NULL grid"),
            (dict(V=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"), (dict(T=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"),
            (dict(h=0.0), "finite and > 0"), (dict(h=-1.0), "finite and > 0"), (dict(h=float("nan")), "finite and > 0"), (dict(h=float("inf")), "finite and > 0"),
            (dict(n=(0, 4, 4)), r"n\[0\] 0 outside \[1, 2\^21\]"), (dict(n=(4, 2 ** 21 + 1, 4)), r"n\[1\] 2097153 outside"), (dict(n=(4, 4, 0)), r"n\[2\] 0 outside"),
            (dict(short=1), "scratch of %d bytes needed, %d given")]
    out = [(e, kw, m) for e in ("count", "emit") for kw, m in both]
    out += [("count", dict(cluster=None), "NULL cluster"), ("count", dict(counts=None), "NULL counts")]
    out += [("emit", dict(nc=1001), "n_clusters 1001 > V 1000"), ("emit", dict(nt=2001), "n_kept_triangles 2001 > T 2000")]
    out += [("emit", {k: None}, "NULL output") for k in ("leader", "members", "positions", "tris_out", "kept")]
    return out


def check_refusals():
    """each rule comes back as AC_ERR_BAD_ARG (1) with its message, before a buffer is touched or anything is launched"""
    from avatarcraft_amd import _lib
    import ctypes
    lib = _lib.lib()
    P = 4096                                                     # a non-NULL address that nothing dereferences
    V, T = 1000, 2000
    need = lib.ac_mesh_cluster_scratch(V, T)

    def call(entry, verts=P, V=V, tris=P, T=T, grid=True, h=1.0, n=(4, 4, 4), scratch=P, nbytes=need, short=0, cluster=P, counts=P, leader=P, members=P,
             positions=P, nc=10, tris_out=P, kept=P, nt=10):
        g = ctypes.byref(_lib.ac_cluster_grid((ctypes.c_double * 3)(0.0, 0.0, 0.0), h, (ctypes.c_uint32 * 3)(*n))) if grid else None
        head = (verts, V, tris, T, g, scratch, nbytes - short)
        if entry == "count":
            return lib.ac_mesh_cluster_count(*head, cluster, counts, None)
        return lib.ac_mesh_cluster_emit(*head, leader, members, positions, nc, tris_out, kept, nt, None)
    for entry, kw, match in refusals():
        assert call(entry, **kw) == 1, (entry, kw)
        err = lib.ac_last_error().decode()
        if "%d" in match:
            match = match % (need, need - 1)
        assert re.search(match, err) and "mesh_cluster_" + entry in err, (entry, kw, err)
    return len(refusals())


def test_every_entry_refuses_before_any_launch():
    assert check_refusals() == 37


# ---------------------------------------------------------------------------------------------------- Python refuses before anything is computed
def test_python_refuses_before_anything_is_computed():
    from avatarcraft_amd import drivers, mesh_decimate
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    g = mesh_decimate.cluster_grid(1.6, 64, 2)
    v, t = torch.zeros((5, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="vertices must be a CUDA tensor"):
        mesh_decimate.mesh_cluster(v, t, g)                                            # CPU tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh_decimate.mesh_cluster(v.numpy(), t, g)
    with pytest.raises(RuntimeError, match="textured mesh"):
        mesh_decimate.decimate_mesh(dict(vertices=v, triangles=t, uv=np.zeros((4, 3, 2))), g)
    with pytest.raises(RuntimeError, match="textured mesh"):
        mesh_decimate.decimate_mesh(dict(vertices=v, triangles=t, texture=np.zeros((8, 8, 3), np.uint8)), g)
    for extra in (dict(normals=torch.zeros(5, 3)), dict(colors=np.zeros((5, 3), np.float32)), dict(sdf=torch.zeros(5), status=torch.zeros(5, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="per-vertex entries \\[%s" % repr(sorted(extra)[0])):
            mesh_decimate.decimate_mesh(dict(vertices=v, triangles=t, **extra), g)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        mesh_decimate.decimate_mesh(dict(vertices=v, triangles=t), g)
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        mesh_decimate.decimate_mesh(dict(vertices=v, triangles=t, component_sizes=torch.zeros((5, 2), dtype=torch.int64)), g)      # not per vertex: not refused for it
    for name in ("extract_geometry", "extract_colored_mesh", "extract_textured_mesh"):
        par = inspect.signature(getattr(NeRFNetwork, name)).parameters
        assert list(par)[-1] == "decimate" and par["decimate"].default is None, name      # the last keyword
    torch.manual_seed(0)
    net = NeRFNetwork()                                                                # on the CPU
    with pytest.raises(RuntimeError, match="decimate"):
        net.extract_geometry(1.6, 16, decimate=2)                                      # the native mesher only: not the CPU's fall-back mesher
    with pytest.raises(RuntimeError, match="decimate"):
        net.extract_geometry(1.6, 16, mesher="tetra", decimate=2)
    for call in (lambda: net.extract_colored_mesh(1.6, 16, decimate=2), lambda: net.extract_textured_mesh(1.6, 16, texture_size=64, decimate=2)):
        with pytest.raises(RuntimeError, match="on the GPU"):
            call()
    for call in (lambda: net.extract_geometry(1.6, 16, decimate=0.5), lambda: net.extract_colored_mesh(1.6, 16, decimate=float("nan")),
                 lambda: net.extract_textured_mesh(1.6, 16, texture_size=64, decimate="2")):
        with pytest.raises((ValueError, RuntimeError), match="cluster_grid: k|decimate"):
            call()
    assert "decimate" in drivers.export_mesh.__doc__ and "decimate" in drivers.export_animation.__doc__
