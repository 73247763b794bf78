"""-m gpu: making the exported mesh manifold on the device -- ac_mesh_repair_count / _emit (csrc/mesh_repair.hip) through the raw entries,
mesh_repair.mesh_repair / repair_mesh, NeRFNetwork.export_manifold and manifold= of drivers.export_mesh -- against the numpy restatement of
tests/mesh_repair_cases.py (which tests/test_mesh_repair_host.py checks against hand-worked meshes).  Everything compared is an integer: every comparison is
exact equality.  The shapes are the smallest at which the kernels can go wrong: hand-worked meshes, soups in which most edges are crowded and hundreds of unites
land on a few words, lattice positions with exact key ties, one edge that every ticket and every claim contends on, edge keys beyond 32 bits, keys that are zero or
not finite, the triangle order under a permutation, decimated and welded marching-cubes meshes.  (mesh_components.hip after the move of its union-find into
mesh_index.hpp: tests/test_gpu_mesh_components.py, untouched.)"""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_component_cases as MC
from tests import mesh_decimate_cases as K
from tests import mesh_repair_cases as R
from tests import mesh_weld_cases as W
from tests.test_gpu_mesh_components import rough_net                                    # noqa: F401 (the fixture: the small network with the rough table)
from tests.test_gpu_mesh_decimate import ATTR_KEYS, BOUND, THRESHOLD, _equal, _shade
from tests.test_gpu_model import DEV

pytestmark = pytest.mark.gpu
KEYS = ("triangles", "source")


def _dev(P, t):
    P = torch.from_numpy(np.ascontiguousarray(np.asarray(P, np.float32).reshape(-1, 3))).to(DEV)
    return P, torch.from_numpy(np.ascontiguousarray(np.asarray(t).reshape(-1, 3))).to(device=DEV, dtype=torch.int32).contiguous()


def _repair(P, t):
    """mesh_repair.mesh_repair -> numpy"""
    from avatarcraft_amd import mesh_repair
    r = mesh_repair.mesh_repair(*_dev(P, t))
    assert set(r) == set(KEYS) | {"report"} and all(r[k].is_cuda for k in KEYS) and tuple(r["report"]) == R.REPORT_KEYS + ("added",)
    assert all(type(x) is int for x in r["report"].values())
    return {k: (x.cpu().numpy() if k in KEYS else x) for k, x in r.items()}


def _same(got, ref):
    assert got["report"] == ref["report"]
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), k


def _raw(P, t, slack=3):
    """the raw entries with outputs `slack` rows longer than needed and poisoned: -> (counts [8], outputs as numpy with the report)"""
    from avatarcraft_amd import _lib as L
    P, t = _dev(P, t)
    V, T = P.shape[0], t.shape[0]
    lib, st = L.lib(), L.current_stream(torch.device(DEV))
    need = int(lib.ac_mesh_repair_scratch(V, T))
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    counts = torch.full((8 + slack,), -7, dtype=torch.int32, device=DEV)
    head = (P.data_ptr() if V else None, t.data_ptr() if T else None, T, V, scratch.data_ptr(), need)
    assert lib.ac_mesh_repair_count(*head, counts.data_ptr(), st) == 0, lib.ac_last_error()
    c = counts.tolist()
    assert c[8:] == [-7] * slack
    nv = c[0]
    full = dict(triangles=torch.full((T + slack, 3), -7, dtype=torch.int32, device=DEV), source=torch.full((nv + slack,), -7, dtype=torch.int32, device=DEV))
    assert lib.ac_mesh_repair_emit(*head, full["triangles"].data_ptr(), full["source"].data_ptr(), nv, st) == 0, lib.ac_last_error()
    torch.cuda.synchronize()
    full = {k: x.cpu().numpy() for k, x in full.items()}
    n = dict(triangles=T, source=nv)
    for k, x in full.items():
        assert (x[n[k]:] == -7).all(), k                                                # nothing is written past the counts
    out = {k: x[:n[k]] for k, x in full.items()}
    out["report"] = dict(zip(R.REPORT_KEYS, c[:8]), added=nv - V)
    return c[:8], out


def _check(P, t, raw=True):
    """the repair of (P, t) through Python (and the raw entries) against the restatement -> the reference"""
    ref = R.repair(P, t)
    if ref["report"]["invalid"] == 0:
        _same(_repair(P, t), ref)
    if raw:
        _same(_raw(P, t)[1], ref)
    return ref


# ---------------------------------------------------------------------------------------------------- degenerate sizes, hand-worked meshes
def test_nothing_and_vertices_alone():
    none = np.zeros((0, 3), np.int32)
    r = _repair(np.zeros((0, 3)), none)                                                  # V = T = 0: legal, nothing is launched
    assert r["triangles"].shape == (0, 3) and r["source"].shape == (0,) and r["report"] == dict.fromkeys(R.REPORT_KEYS + ("added",), 0)
    counts, out = _raw(np.zeros((0, 3)), none)
    assert counts == [0] * 8
    ref = _check(np.zeros((5, 3)), none)                                                 # vertices and no triangle: every vertex keeps its index
    assert ref["source"].tolist() == [0, 1, 2, 3, 4]
    ref = _check(R.random_positions(3), [[0, 1, 2]])
    assert ref["report"]["added"] == 0
    ref = _check(R.random_positions(5), [[4, 2, 2]])                                     # one degenerate triangle: copied
    assert ref["report"]["degenerate"] == 1 and ref["triangles"].tolist() == [[4, 2, 2]]


def test_the_hand_worked_meshes():
    ref = _check(*R.two_tetrahedra_on_an_edge())
    assert ref["report"]["added"] == 2 and ref["source"][6:].tolist() == [0, 1] and W.topology(ref["triangles"], 8)["closed_manifold"]
    ref = _check(*R.two_tetrahedra_on_a_vertex())
    assert (ref["report"]["added"], ref["report"]["nonmanifold"], ref["report"]["split"]) == (1, 0, 1)
    ref = _check(*R.fin())
    assert (ref["report"]["cut"], ref["report"]["paired"]) == (1, 2)
    ref = _check(*R.one_edge(10))
    assert (ref["report"]["crowded"], ref["report"]["cut"]) == (1, 10)
    for n in (3, 4, 7, 8, 9):                                                            # around the threshold between ordered and crowded
        ref = _check(*R.one_edge(n, seed=n))
        assert ref["report"]["crowded"] == (n > 8) and ref["report"]["paired"] + ref["report"]["cut"] == n


def test_keys_that_are_zero_tie_or_are_not_finite():
    P, t = R.fin()
    Q = P.copy()
    Q[4] = Q[2]                                                                          # equal keys: the use id decides
    assert _check(Q, t)["report"]["paired"] == 2
    Q = P.copy()
    Q[1] = Q[0]                                                                          # a zero-length edge: s == 0 for every use
    assert _check(Q, t)["report"]["crowded"] == 0
    Q = P.copy()
    Q[3] = Q[0] + 0.25 * (Q[1] - Q[0])                                                   # a zero-area reference triangle ...
    for tri in ([[0, 1, 3], [1, 0, 2], [0, 1, 4]], [[1, 0, 3], [0, 1, 2], [0, 1, 4], [1, 0, 2]]):
        ref = _check(Q, tri)                                                             # ... its opposite vertex lies on the edge: w = 0, every key is 0
        assert ref["report"]["nonmanifold"] == 1 and ref["report"]["crowded"] == 0
    for bad in (np.nan, np.inf):
        Q = P.copy()
        Q[4, 1] = bad                                                                    # a position that is not finite: the edge is treated as crowded
        ref = _check(Q, t)
        assert (ref["report"]["crowded"], ref["report"]["cut"], ref["report"]["paired"]) == (1, 3, 0)
    Q = (P * np.float32(3e37)).astype(np.float32)                                        # finite positions, keys from products that overflow fp32 but not fp64
    assert _check(Q, t)["report"]["crowded"] == 0


# ---------------------------------------------------------------------------------------------------- soups: contention, ties, long keys, the order
@pytest.mark.parametrize("V,T", [(12, 63), (12, 257), (12, 1025), (12, 2049), (40, 300), (40, 1500)])
def test_random_soups_over_a_few_vertices(V, T):
    """V = 12: 66 edges, so from T = 257 on most edges are crowded and every unite of the mesh lands on a few words; V = 40: 780 edges with 1 to 8 uses at
    T = 300 and around the threshold at T = 1500.  Sizes on both sides of a wave, a workgroup and the 1024 corners of a scanned workgroup"""
    P, t = R.soup(V, T, seed=T)
    rep = _check(P, t)["report"]
    assert rep["degenerate"] > 0 and rep["nonmanifold"] > 0 and rep["added"] > 0          # no case passes vacuously
    if V == 12 and T >= 257:
        assert rep["crowded"] > rep["nonmanifold"] // 2
    if V == 40:
        assert rep["paired"] > 0 and rep["cut"] > 0 and rep["nonmanifold"] > rep["crowded"]


@pytest.mark.parametrize("V,T,lattice", [(300, 2000, 3), (300, 1500, 2), (200, 2500, 4)])
def test_soups_on_the_integer_lattice(V, T, lattice):
    """positions on a tiny integer lattice: coincident points, coplanar uses, exact key ties and zero keys on most edges"""
    P, t = R.soup(V, T, seed=V + T, lattice=lattice)
    rep = _check(P, t)["report"]
    assert rep["paired"] > 0 and rep["cut"] > 0 and rep["nonmanifold"] > rep["crowded"]


def test_every_triangle_on_one_edge():
    """all tickets, all claims and both ends' unites on one slot: crowded with many uses, ordered with eight"""
    ref = _check(*R.one_edge(5000, seed=7), raw=False)
    assert ref["report"]["crowded"] == 1 and ref["report"]["cut"] == 5000 and ref["report"]["added"] == 2 * 4999
    P, t = R.one_edge(8, seed=8)
    ref = _check(P, np.concatenate([t, W.random_triangles(10, 0)]))
    assert ref["report"]["nonmanifold"] == 1 and ref["report"]["crowded"] == 0
    ref = _check(*R.one_edge(3000, seed=9, V=40), raw=False)                              # third corners from 38 vertices: their edges are crowded as well
    assert ref["report"]["crowded"] > 40


def test_edge_keys_beyond_32_bits():
    t, V = W.high_indices()
    ref = _check(R.random_positions(V, seed=1), t)
    assert ref["report"]["nonmanifold"] == 779 and ref["report"]["crowded"] > 0 and ref["report"]["paired"] > 0 and ref["report"]["split"] == 40
    t, V = W.high_indices(T=400, pool=60)
    ref = _check(R.random_positions(V, seed=2), t)
    assert ref["report"]["paired"] > 0 and ref["report"]["cut"] > 0
    t, V = W.low_word_twins()                                                            # edges that agree in the low 32 bits of their key
    ref = _check(R.random_positions(V, seed=3), t)
    assert (ref["report"]["nonmanifold"], ref["report"]["paired"], ref["report"]["crowded"]) == (3, 12, 0)   # the shared face's three edges, four uses each


def test_the_result_follows_the_use_ids_not_the_arrival():
    for P, t in (R.soup(40, 1500, seed=1500), R.soup(300, 2000, seed=2300, lattice=3)):
        pt, p = W.permuted_triangles(t)
        got, ref = _repair(P, pt), R.repair(P, pt)
        _same(got, ref)
        plain = _repair(P, t)
        assert plain["report"]["nonmanifold"] == got["report"]["nonmanifold"] and plain["report"]["crowded"] == got["report"]["crowded"]


def test_two_runs_are_identical():
    for P, t in (R.soup(12, 2049, seed=2049), R.soup(40, 1500, seed=1500), _welded("noise")):
        _same(_repair(P, t), _repair(P, t))


# ---------------------------------------------------------------------------------------------------- decimated, welded marching-cubes meshes
@functools.lru_cache(maxsize=None)
def _welded(name, k=None):
    """a marching-cubes case decimated and welded by the restatements (the device's own marching cubes gives the oracle's mesh: tests/test_gpu_geometry.py)"""
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.mesh_decimate import cluster_grid
    mc = lambda u, **kw: tuple(x.cpu().numpy() for x in nsr_ops.marching_cubes(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(DEV), 0.0, **kw))
    if name == "noise":
        v, t = mc(MC.noise_volumes()[0])
        return R.welded(v, t, K.grid_over(v.min(axis=0) - 1e-3, v.max(axis=0) + 1e-3, 2.0))
    n, u = (32, R.shell_volume(32)) if name == "shell" else (40, MC.body_with_floaters(40))
    v, t = mc(u, den=n - 1.0, span=[2.0] * 3, lo=[-1.0] * 3)
    return R.welded(v, t, cluster_grid(1.0, n, k))


@pytest.mark.parametrize("k,size,nonmanifold,added,paired,closed", [(3, (214, 556), (82, 0), 132, 328, True), (2, (524, 1336), (144, 3), 174, 576, False)])
def test_the_thin_shell(k, size, nonmanifold, added, paired, closed):
    P, t = _welded("shell", k)
    assert (len(P), len(t)) == size
    ref = _check(P, t)
    rep, after = ref["report"], W.topology(ref["triangles"], ref["report"]["vertices"])
    assert (rep["nonmanifold"], rep["added"], rep["paired"], rep["cut"]) == (nonmanifold[0], added, paired, 0)
    assert (after["nonmanifold"], after["boundary"], after["closed_manifold"]) == (nonmanifold[1], 0, closed)
    again = _repair(P[ref["source"]], ref["triangles"])                                   # idempotent
    assert again["report"]["added"] == 0 and np.array_equal(again["triangles"], ref["triangles"])


def test_the_noise_volume():
    P, t = _welded("noise")
    assert (len(P), len(t)) == (3350, 13846)
    ref = _check(P, t)
    rep, after = ref["report"], W.topology(ref["triangles"], ref["report"]["vertices"])
    assert (rep["nonmanifold"], rep["added"], rep["cut"], rep["paired"]) == (3028, 3167, 84, 12336) and (after["nonmanifold"], after["boundary"]) == (237, 76)
    again = _repair(P[ref["source"]], ref["triangles"])
    assert again["report"]["added"] == 0 and np.array_equal(again["triangles"], ref["triangles"])


@pytest.mark.parametrize("k", [2, 3, 5])
def test_the_floater_meshes_come_back_unchanged(k):
    P, t = _welded("floaters", k)
    ref = _check(P, t)
    assert ref["report"]["added"] == 0 and np.array_equal(ref["triangles"], t)


# ---------------------------------------------------------------------------------------------------- invalid triangles, refusals
def test_invalid_triangles_are_counted_and_refused_by_python():
    from avatarcraft_amd import mesh_repair
    P, t = _welded("shell", 3)
    V = len(P)
    extra = np.array([[-1, 1, 2], [3, V, 4], [6, 8, -2147483648], [2147483647, 9, 10], [V - 2, V - 3, V]], np.int32)
    mixed = np.concatenate([t[:100], extra, t[100:]]).astype(np.int32)
    ref = R.repair(P, mixed)
    assert ref["report"]["invalid"] == 5 and ref["report"]["added"] == 132
    counts, out = _raw(P, mixed)
    _same(out, ref)
    assert np.array_equal(out["triangles"][100:105], extra)                              # copied as they stand
    with pytest.raises(RuntimeError, match=r"mesh_repair: 5 of %d triangles name an index outside \[0, %d\) \(counts: \{'vertices'" % (len(mixed), V)):
        mesh_repair.mesh_repair(*_dev(P, mixed))
    with pytest.raises(RuntimeError, match="triangles over no vertex"):
        mesh_repair.mesh_repair(*_dev(np.zeros((0, 3)), t))


def test_every_entry_refuses_before_any_launch():
    from tests.test_mesh_repair_host import check_refusals
    assert check_refusals() == 21
    torch.cuda.synchronize()                                                            # (nothing was launched: nothing can have gone wrong on the device)


def test_repair_mesh_gathers_what_is_per_vertex():
    from avatarcraft_amd.mesh_repair import repair_mesh
    P, t = _welded("shell", 3)
    ref = R.repair(P, t)
    V = len(P)
    Pd, td = _dev(P, t)
    mesh = dict(vertices=Pd.double(), triangles=td, cluster=torch.arange(V, device=DEV, dtype=torch.int32), cluster_members=torch.arange(V, device=DEV, dtype=torch.int32) + 1,
                normals=torch.arange(3 * V, device=DEV, dtype=torch.float32).reshape(V, 3), component_sizes=torch.zeros((V, 2), dtype=torch.int64, device=DEV))
    got = repair_mesh(mesh)
    src = torch.from_numpy(ref["source"]).long().to(DEV)
    assert set(got) == set(mesh) | {"repair"} and got["repair"] == ref["report"]
    assert np.array_equal(got["triangles"].cpu().numpy(), ref["triangles"]) and got["vertices"].dtype == torch.float64
    assert torch.equal(got["vertices"], mesh["vertices"][src]) and torch.equal(got["normals"], mesh["normals"][src])
    assert torch.equal(got["cluster_members"], mesh["cluster_members"][src])
    assert got["cluster"] is mesh["cluster"] and got["component_sizes"] is mesh["component_sizes"]            # old indices stay valid; not per vertex: carried over
    with pytest.raises(RuntimeError, match="textured mesh"):
        repair_mesh(dict(got, uv=torch.zeros((len(t), 3, 2), device=DEV)))


# ---------------------------------------------------------------------------------------------------- model level
# the rough-field recipe of tests/test_gpu_mesh_components.py at the smallest resolution and k that leave non-manifold edges after the weld: on the CPU oracle's grids
# 16^3 leaves none at k = 2, 3, 4; 24^3 at k = 2 leaves 3 (39 vertices / 78 triangles after the weld; the repair removes all three and adds 2 vertices)
RES, KD = 24, 2


class _switches:
    """net.export_weld = True (and net.export_manifold = manifold) inside the block"""
    def __init__(self, net, manifold):
        self.net, self.manifold = net, manifold

    def __enter__(self):
        self.net.export_weld = True
        if self.manifold:
            self.net.export_manifold = True

    def __exit__(self, *exc):
        del self.net.export_weld
        if self.manifold:
            del self.net.export_manifold


@pytest.fixture(scope="module")
def welded_by_the_model(rough_net):
    """the parent behaviour: the welded, shaded mesh with the switch off"""
    assert rough_net.export_manifold is False
    with _switches(rough_net, False):
        return rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)


def test_switch_on_is_the_restatement_of_the_welded_mesh(rough_net, welded_by_the_model):
    from avatarcraft_amd.mesh_decimate import cluster_grid
    from avatarcraft_amd.mesh_weld import mesh_topology
    off = welded_by_the_model
    with _switches(rough_net, False):
        v, t = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)       # the device's own welded mesh, before the shading
    assert torch.equal(t, off["triangles"])
    ref = R.repair(v.cpu().numpy(), t.cpu().numpy())
    before = mesh_topology(t, v.shape[0])
    assert before["nonmanifold"] > 0 and ref["report"]["added"] > 0                        # no vacuous pass: there is something to repair
    with _switches(rough_net, True):
        got = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
        vg, tg = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
        with pytest.raises(RuntimeError, match="export_manifold|export_weld"):
            rough_net.extract_geometry(BOUND, 32, mesher="tetra")
    assert rough_net.export_manifold is False
    assert set(got) == set(off) | {"repair"} and got["repair"] == ref["report"] and got["weld"] == off["weld"]
    assert np.array_equal(got["triangles"].cpu().numpy(), ref["triangles"]) and torch.equal(tg, got["triangles"])
    src = torch.from_numpy(ref["source"]).long().to(DEV)
    assert torch.equal(vg.view(torch.int64), v[src].view(torch.int64)) and torch.equal(got["cluster_members"], off["cluster_members"][src])
    _equal(got, {k: off[k][src] for k in ATTR_KEYS}, ATTR_KEYS)                            # the copies are shaded like the vertex they copy: coincident
    _equal(got, _shade(rough_net, vg, cluster_grid(BOUND, RES, KD)["h"]), ATTR_KEYS)
    after = mesh_topology(got["triangles"], got["vertices"].shape[0])
    assert after == W.topology(ref["triangles"], ref["report"]["vertices"])
    assert before["boundary"] == 0 and after["boundary"] <= got["repair"]["cut"]           # no boundary beyond the cut uses
    assert after["nonmanifold"] < before["nonmanifold"] and after["faces"] == before["faces"]


def test_switch_off_is_what_it_was(rough_net, welded_by_the_model):
    from avatarcraft_amd.mesh_decimate import cluster_grid, decimate_mesh
    from avatarcraft_amd.mesh_weld import weld_mesh
    v, t = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True)
    g = cluster_grid(BOUND, RES, KD)
    dm = decimate_mesh(dict(vertices=v, triangles=t), g)
    wm = weld_mesh(dm)
    off = welded_by_the_model
    assert set(off) == {"vertices", "triangles", "normals", "colors", "sdf", "status", "cluster_members", "weld"}       # exactly the parent's keys: no report
    _equal(off, _shade(rough_net, wm["vertices"], g["h"]), ATTR_KEYS)
    assert torch.equal(off["triangles"], wm["triangles"]) and torch.equal(off["cluster_members"], wm["cluster_members"]) and off["weld"] == wm["weld"]
    plain = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)             # neither switch
    assert set(plain) == {"vertices", "triangles", "normals", "colors", "sdf", "status", "cluster_members"}
    _equal(plain, _shade(rough_net, dm["vertices"], g["h"]), ATTR_KEYS)
    assert torch.equal(plain["triangles"], dm["triangles"])


def test_manifold_without_the_weld_and_with_a_texture(rough_net):
    from avatarcraft_amd.geometry import atlas_layout, clean_mesh
    from avatarcraft_amd.mesh_decimate import cluster_grid, decimate_mesh
    v, t = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True)
    dm = decimate_mesh(dict(vertices=v, triangles=t), cluster_grid(BOUND, RES, KD))
    ref = R.repair(dm["vertices"].cpu().numpy(), dm["triangles"].cpu().numpy())
    rough_net.export_manifold = True
    try:
        vg, tg = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)   # after the decimation when the weld is off
        tex = rough_net.extract_textured_mesh(BOUND, RES, texture_size=512, threshold=THRESHOLD, return_torch=True, decimate=KD)
    finally:
        del rough_net.export_manifold
    assert np.array_equal(tg.cpu().numpy(), ref["triangles"]) and vg.shape[0] == ref["report"]["vertices"]
    assert tex["repair"] == ref["report"] and "weld" not in tex and torch.equal(tex["triangles"], tg)
    assert np.array_equal(tex["uv"].cpu().numpy(), atlas_layout(len(ref["triangles"]), 512)["uv"])             # every triangle keeps its place: the same atlas
    cleaned = clean_mesh(dict(vertices=vg, triangles=tg), "largest")                                           # the repaired mesh goes through the cleaning
    assert 0 < cleaned["triangles"].shape[0] <= tg.shape[0]


def test_the_driver_writes_the_repaired_mesh_and_reports_its_topology(rough_net, welded_by_the_model, tmp_path):
    from avatarcraft_amd import drivers
    from tests.test_mesh_export_host import read_ply
    off = welded_by_the_model
    path = str(tmp_path / "manifold.ply")
    mesh = drivers.export_mesh(rough_net, path, bound=BOUND, resolution=RES, threshold=THRESHOLD, decimate=KD, weld=True, manifold=True)
    assert rough_net.export_weld is False and rough_net.export_manifold is False
    props, table, faces, size = read_ply(path)
    T = off["triangles"].shape[0]
    assert len(faces) == T and len(table) == mesh["repair"]["vertices"] and mesh["repair"]["added"] > 0 and mesh["weld"] == off["weld"]
    assert np.array_equal(np.asarray(faces), mesh["triangles"])
    assert mesh["topology"] == W.topology(mesh["triangles"], mesh["repair"]["vertices"]) and mesh["topology"]["faces"] == T
    plain = drivers.export_mesh(rough_net, str(tmp_path / "welded.ply"), bound=BOUND, resolution=RES, threshold=THRESHOLD, decimate=KD, weld=True)
    assert "repair" not in plain and plain["topology"]["nonmanifold"] > mesh["topology"]["nonmanifold"]
    assert plain["topology"]["boundary"] == 0 and mesh["topology"]["boundary"] <= mesh["repair"]["cut"]
    only = drivers.export_mesh(rough_net, str(tmp_path / "only.ply"), bound=BOUND, resolution=RES, threshold=THRESHOLD, decimate=KD, manifold=True)
    assert "weld" not in only and "topology" in only and only["repair"]["added"] > 0
