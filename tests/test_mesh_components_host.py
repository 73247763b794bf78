"""CPU tier of the mesh cleaning (ac_mesh_components / ac_mesh_compact_count / _emit, csrc/mesh_components.hip; nsr_ops.mesh_components / mesh_compact;
geometry.select_components / clean_mesh; components= of the model's extractors): the entries and their refusals, which come before any launch and so run without
a device; the selection rules on hand-written size tables; the yardstick of the GPU tier (tests/mesh_component_cases.py) against scipy; and the Python-level
refusals, which come before anything is computed.  The GPU tier (tests/test_gpu_mesh_components.py) compares the kernels with the yardstick, exactly."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_component_cases as K

NAMES = ("ac_mesh_components_scratch", "ac_mesh_components", "ac_mesh_compact_scratch", "ac_mesh_compact_count", "ac_mesh_compact_emit")


def test_the_entries_are_declared_and_bound():
    from avatarcraft_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avatarcraft_hip.h")).read()
    for name, ret, arity in zip(NAMES, ("size_t", "int", "size_t", "int", "int"), (2, 11, 2, 10, 15)):
        assert name in _lib.EXPORTS and re.search(r"\b%s %s\s*\(" % (ret, name), hdr)
        assert len(_lib._SIGS[name][0]) == arity
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == arity                  # the header's parameter list and the binding's agree
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().ac_version() == 10                                                              # added entries, no struct changed


def test_scratch_sizes_are_host_functions():
    from avatarcraft_amd import _lib
    lib = _lib.lib()
    cc, cp = lib.ac_mesh_components_scratch, lib.ac_mesh_compact_scratch
    assert cc(2 ** 31, 0) == 0 and cc(0, 2 ** 31) == 0 and cp(2 ** 31, 0) == 0 and cp(0, 2 ** 31) == 0      # indices are int32
    V, T = 1_580_000, 3_160_000                                                                              # the 2048^3 streamed export
    assert 4 * V <= cc(V, T) < 4.1 * V                                                                       # parent[V] and the scans' per-workgroup words
    assert 0 < cp(V, T) < 0.02 * 12 * T                                                                      # the compaction keeps per-workgroup words only
    assert cc(2 ** 31 - 1, 2 ** 31 - 1) > 0 and cp(2 ** 31 - 1, 2 ** 31 - 1) > 0
    assert cc(0, 0) >= 0 and cp(0, 0) >= 0
    assert cc(1000, 10) <= cc(1001, 10) and cp(10, 2000) >= cp(10, 1000)


def test_every_entry_refuses_before_any_launch():
    """AC_ERR_BAD_ARG (1) comes back with its message before a buffer is touched or anything is launched: this runs without a device (the addresses are never read)"""
    from avatarcraft_amd import _lib
    lib = _lib.lib()
    P = 4096                                                     # a non-NULL address that nothing dereferences
    V, T, C = 1000, 2000, 7
    need_cc, need_cp = lib.ac_mesh_components_scratch(V, T), lib.ac_mesh_compact_scratch(V, T)

    def label(tris=P, T=T, V=V, root=P, comp=P, sizes=P, maxc=V, counts=P, scratch=P, nbytes=need_cc):
        return lib.ac_mesh_components(tris, T, V, root, comp, sizes, maxc, counts, scratch, nbytes, None)

    def count(tris=P, T=T, V=V, comp=P, keep=P, C=C, scratch=P, nbytes=need_cp, counts=P):
        return lib.ac_mesh_compact_count(tris, T, V, comp, keep, C, scratch, nbytes, counts, None)

    def emit(tris=P, T=T, V=V, comp=P, keep=P, C=C, scratch=P, nbytes=need_cp, vmap=P, kv=P, nkv=10, to=P, kt=P, nkt=10):
        return lib.ac_mesh_compact_emit(tris, T, V, comp, keep, C, scratch, nbytes, vmap, kv, nkv, to, kt, nkt, None)
    err = lambda: lib.ac_last_error().decode()
    for kw, match in ((dict(tris=None), "NULL"), (dict(root=None), "NULL"), (dict(comp=None), "NULL"), (dict(sizes=None), "NULL"), (dict(counts=None), "NULL counts"),
                      (dict(scratch=None), "NULL"), (dict(V=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"), (dict(T=2 ** 31), r"above 2\^31 - 1"),
                      (dict(nbytes=need_cc - 1), "scratch of %d bytes needed, %d given" % (need_cc, need_cc - 1)), (dict(V=0, T=5), "5 triangles over no vertex")):
        assert label(**kw) == 1, kw
        assert re.search(match, err()) and "mesh_components" in err(), (kw, err())
    for fn in (count, emit):
        for kw, match in ((dict(tris=None), "NULL"), (dict(comp=None), "NULL"), (dict(keep=None), "NULL"), (dict(scratch=None), "NULL"),
                          (dict(V=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"), (dict(T=2 ** 31, nbytes=2 ** 40), r"above 2\^31 - 1"),
                          (dict(nbytes=need_cp - 1), "scratch of %d bytes needed, %d given" % (need_cp, need_cp - 1)), (dict(C=V + 1), "C 1001 > V 1000"),
                          (dict(V=0, T=5, C=0), "5 triangles over no vertex")):
            assert fn(**kw) == 1, (fn.__name__, kw)
            assert re.search(match, err()) and "mesh_compact" in err(), (kw, err())
    assert count(counts=None) == 1 and "NULL counts" in err()
    for kw, match in ((dict(nkv=V + 1), "n_kept_vertices 1001 > V 1000"), (dict(nkt=T + 1), "n_kept_triangles 2001 > T 2000"), (dict(vmap=None), "NULL output"),
                      (dict(kv=None), "NULL output"), (dict(to=None), "NULL output"), (dict(kt=None), "NULL output")):
        assert emit(**kw) == 1 and re.search(match, err()), (kw, err())


def test_the_yardstick_agrees_with_scipy_up_to_relabelling():
    """tests/mesh_component_cases.components (a serial union-find with root = minimum) against scipy.sparse.csgraph.connected_components on the cases of the GPU tier
    that need no device: the partitions are equal, and the yardstick's own labelling is the canonical one"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rs = np.random.RandomState(5)
    soup = rs.randint(0, 400, (150, 3)).astype(np.int32)                              # random triangles: shared vertices, isolated vertices, a few degenerate ones
    soup[::17, 1] = soup[::17, 0]
    for tris, V in (K.strip(257, "permuted", shuffle_triangles=True), K.strip(1025, "descending"), K.fan(500), K.disjoint(300), (soup, 400),
                    (np.zeros((0, 3), np.int32), 5)):
        r = K.components(tris, V)
        e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
        n, lab = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V)), directed=False)
        assert n == r["n_components"] and r["n_bad"] == 0
        pairs = np.unique(np.stack([lab, r["component"]], axis=1), axis=0)
        assert len(pairs) == n                                                        # a bijection between the two labellings
        for c in range(n):
            members = np.flatnonzero(r["component"] == c)
            assert (r["root"][members] == members.min()).all()
        assert np.array_equal(np.unique(r["root"]), np.flatnonzero(r["root"] == np.arange(V)))
        assert (np.diff(np.unique(r["root"])) > 0).all() and np.array_equal(r["component"][np.unique(r["root"])], np.arange(n))
        assert r["sizes"][:, 0].sum() == V and r["sizes"][:, 1].sum() == len(tris)
    bad = np.array([[0, 1, 2], [2, 3, -1], [4, 5, 6], [6, 7, 8], [5, 9, 9]], np.int32)  # (2, 3, -1) and (5, 9, 9) with V = 9 are invalid and join nothing
    r = K.components(bad, 9)
    assert r["n_bad"] == 2 and r["root"].tolist() == [0, 0, 0, 3, 4, 4, 4, 4, 4] and r["sizes"].tolist() == [[3, 1], [1, 0], [5, 2]]
    c = K.compact(bad, r["component"], [False, True, True])
    assert c["vertex_map"].tolist() == [-1, -1, -1, 0, 1, 2, 3, 4, 5] and c["triangles"].tolist() == [[1, 2, 3], [3, 4, 5]] and c["kept_triangles"].tolist() == [2, 3]


def test_select_components_rules():
    from avatarcraft_amd.geometry import select_components
    sizes = np.array([[10, 5], [40, 70], [3, 1], [41, 70], [1, 0], [30, 12]])          # components 1 and 3 tie at 70 triangles
    sel = lambda spec: select_components(sizes, spec).tolist()
    assert sel("largest") == [False, True, False, False, False, False]                # the tie goes to the lower component id
    assert sel(("largest", 1)) == sel("largest")
    assert sel(("largest", 2)) == [False, True, False, True, False, False]
    assert sel(("largest", 3)) == [False, True, False, True, False, True]
    assert sel(("largest", 0)) == [False] * 6 and sel(("largest", 6)) == [True] * 6 and sel(("largest", 99)) == [True] * 6       # k larger than C: all
    assert sel(("min_faces", 12)) == [False, True, False, True, False, True] and sel(("min_faces", 0)) == [True] * 6
    assert sel(("min_faces", 71)) == [False] * 6                                      # keeping none is legal
    mask = np.array([True, False, False, False, True, False])
    assert sel(mask) == mask.tolist() and sel(mask.tolist()) == mask.tolist() and sel(torch.from_numpy(mask)) == mask.tolist()
    assert sel(lambda s: s[:, 0] > 20) == [False, True, False, True, False, True]     # a callable on the table
    assert select_components(torch.from_numpy(sizes), "largest").dtype == bool
    assert select_components(np.zeros((0, 2), np.int64), "largest").shape == (0,)
    for bad in ("smallest", ("largest",), ("largest", -1), ("largest", 1.5), ("largest", True), ("min_faces", "3"), ("area", 2), ("largest", 1, 2), None, 3, 0.5,
                mask[:5], np.ones(7, bool), np.ones(6, np.int32), np.ones((6, 1), bool), lambda s: np.ones(3, bool), lambda s: "largest"):
        with pytest.raises(ValueError, match="select_components"):
            select_components(sizes, bad)


def test_python_refuses_before_anything_is_computed():
    from avatarcraft_amd import geometry, nsr_ops
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    tris = torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        nsr_ops.mesh_components(tris, 5)                                               # CPU tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        nsr_ops.mesh_compact(tris, torch.zeros(5, dtype=torch.int32), torch.ones(1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        nsr_ops.mesh_components(tris.numpy(), 5)
    with pytest.raises(RuntimeError, match="textured mesh"):
        geometry.clean_mesh(dict(vertices=torch.zeros(5, 3), triangles=tris, uv=np.zeros((4, 3, 2))), "largest")
    with pytest.raises(RuntimeError, match="textured mesh"):
        geometry.clean_mesh(dict(vertices=torch.zeros(5, 3), triangles=tris, texture=np.zeros((8, 8, 3), np.uint8)), "largest")
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        geometry.clean_mesh(dict(vertices=torch.zeros(5, 3), triangles=tris), "largest")
    for name in ("extract_geometry", "extract_colored_mesh", "extract_textured_mesh"):
        par = inspect.signature(getattr(NeRFNetwork, name)).parameters
        assert "components" in par and par["components"].default is None, name
    torch.manual_seed(0)
    net = NeRFNetwork()                                                                # on the CPU
    with pytest.raises(RuntimeError, match="components"):
        net.extract_geometry(1.6, 16, components="largest")                            # the native mesher only: not the CPU's fall-back mesher
    with pytest.raises(RuntimeError, match="components"):
        net.extract_geometry(1.6, 16, mesher="tetra", components="largest")
    for call in (lambda: net.extract_colored_mesh(1.6, 16, components="largest"), lambda: net.extract_textured_mesh(1.6, 16, texture_size=64, components="largest")):
        with pytest.raises(RuntimeError, match="on the GPU"):
            call()
    from avatarcraft_amd import drivers
    assert "components" in drivers.export_mesh.__doc__ and "components" in drivers.export_animation.__doc__
