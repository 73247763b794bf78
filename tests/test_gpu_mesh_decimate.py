"""-m gpu: decimating the exported mesh on the device -- ac_mesh_cluster_count / _emit (csrc/mesh_cluster.hip) through the raw entries, mesh_decimate.mesh_cluster /
decimate_mesh and decimate= of the model's extractors -- against the numpy restatement of tests/mesh_decimate_cases.py (which tests/test_mesh_decimate_host.py
checks against hand-worked meshes).  Everything compared is an integer or a function of exact integer sums evaluated in one fixed order in fp64: every comparison
is exact equality, positions included.  The shapes are the smallest at which the kernels can go wrong: the sizes around a wave, a workgroup and the 1024 items of a
scanned workgroup, one slot that every add contends on, keys beyond 2^32, ids under a permutation, real marching-cubes meshes."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_component_cases as MC
from tests import mesh_decimate_cases as K
from tests.test_gpu_mesh_components import rough_net                                    # noqa: F401 (the fixture: the small network with the rough table)
from tests.test_gpu_model import DEV

pytestmark = pytest.mark.gpu
KEYS = ("cluster", "leader", "members", "positions", "triangles", "kept_triangles")


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt).contiguous()


def _cluster(v, t, g):
    """mesh_decimate.mesh_cluster -> numpy"""
    from avatarcraft_amd import mesh_decimate
    r = mesh_decimate.mesh_cluster(_dev(np.asarray(v, np.float64).reshape(-1, 3), torch.float64), _dev(np.asarray(t).reshape(-1, 3), torch.int32), g)
    assert set(r) == set(KEYS) and all(x.is_cuda for x in r.values())
    return {k: x.cpu().numpy() for k, x in r.items()}


def _same(got, ref):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert got[k].tobytes() == ref[k].tobytes(), k                                  # (bytes: -0.0 and the last bit of a position count)


def _raw(v, t, g, slack=3):
    """the raw entries with outputs `slack` rows longer than needed and poisoned: -> (counts [4], outputs as numpy, whole buffers)"""
    import ctypes as C
    from avatarcraft_amd import _lib as L
    v, t = _dev(np.asarray(v, np.float64).reshape(-1, 3), torch.float64), _dev(np.asarray(t).reshape(-1, 3), torch.int32)
    V, T = v.shape[0], t.shape[0]
    grid = L.ac_cluster_grid((C.c_double * 3)(*g["lo"]), g["h"], (C.c_uint32 * 3)(*g["n"]))
    need = int(L.lib().ac_mesh_cluster_scratch(V, T))
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    cluster = torch.full((V + slack,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    st = L.current_stream(torch.device(DEV))
    head = (v.data_ptr() if V else None, V, t.data_ptr() if T else None, T, C.byref(grid), scratch.data_ptr(), need)
    assert L.lib().ac_mesh_cluster_count(*head, cluster.data_ptr(), counts.data_ptr(), st) == 0, L.lib().ac_last_error()
    nc, nt, bad_v, bad_t = counts.tolist()
    leader = torch.full((nc + slack,), -7, dtype=torch.int32, device=DEV)
    members = torch.full((nc + slack,), -7, dtype=torch.int32, device=DEV)
    positions = torch.full((nc + slack, 3), -7.0, dtype=torch.float64, device=DEV)
    tris = torch.full((nt + slack, 3), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((nt + slack,), -7, dtype=torch.int32, device=DEV)
    assert L.lib().ac_mesh_cluster_emit(*head, leader.data_ptr(), members.data_ptr(), positions.data_ptr(), nc, tris.data_ptr(), kept.data_ptr(), nt, st) == 0
    torch.cuda.synchronize()
    full = dict(cluster=cluster, leader=leader, members=members, positions=positions, triangles=tris, kept_triangles=kept)
    full = {k: x.cpu().numpy() for k, x in full.items()}
    n = dict(cluster=V, leader=nc, members=nc, positions=nc, triangles=nt, kept_triangles=nt)
    for k, x in full.items():
        assert (x[n[k]:] == -7).all(), k                                                # nothing is written past the counts
    return (nc, nt, bad_v, bad_t), {k: x[:n[k]] for k, x in full.items()}


def _gpu_mc(u, iso, **kw):
    from avatarcraft_amd import nsr_ops
    v, t = nsr_ops.marching_cubes(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(DEV), iso, **kw)
    return v.cpu().numpy(), t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mc_case(name):
    """(vertices, triangles, volume shape, transform) of a marching-cubes mesh, made once on the device"""
    padded, (opened, kw) = MC.noise_volumes()
    u, iso, kw = {"noise_iso0": (padded, 0.0, {}), "open_noise": (opened, 0.2, kw), "floaters": (MC.body_with_floaters(), 0.0, {})}[name]
    v, t = _gpu_mc(u, iso, **kw)
    return v, t, u.shape, kw


# ---------------------------------------------------------------------------------------------------- degenerate sizes
def test_nothing_one_triangle_and_cells_of_their_own():
    g = K.grid(0.0, 1.0, 4)
    r = _cluster(np.zeros((0, 3)), np.zeros((0, 3), np.int32), g)                        # V = T = 0: legal, nothing is launched
    assert all(r[k].size == 0 for k in KEYS) and r["positions"].shape == (0, 3) and r["triangles"].shape == (0, 3)
    counts, raw = _raw(np.zeros((0, 3)), np.zeros((0, 3), np.int32), g)
    assert counts == (0, 0, 0, 0)
    v, t = [[1.25, 1.5, 1.75], [1.5, 1.5, 1.5], [1.75, 1.25, 1.0]], [[0, 1, 2]]            # one triangle in one cell: one cluster, no triangle
    r = _cluster(v, t, g)
    _same(r, K.cluster(v, t, g))
    assert r["cluster"].tolist() == [0, 0, 0] and r["leader"].tolist() == [0] and r["members"].tolist() == [3]
    assert r["positions"][0, 0] == 1.5 and r["triangles"].shape == (0, 3) and r["kept_triangles"].shape == (0,)
    r = _cluster(v, np.zeros((0, 3), np.int32), g)                                       # vertices and no triangle
    _same(r, K.cluster(v, np.zeros((0, 3), np.int32), g))
    v, t, g = K.own_cells(3000)                                                          # every vertex in a cell of its own: nothing merges, nothing is dropped
    r = _cluster(v, t, g)
    _same(r, K.cluster(v, t, g))
    assert np.array_equal(r["cluster"], np.arange(3000)) and np.array_equal(r["triangles"], t) and (r["members"] == 1).all()
    assert r["positions"].tobytes() == v.tobytes()                                       # a cluster of one: its own vertex, bit for bit (offsets of 0.5 are exact)


# ---------------------------------------------------------------------------------------------------- the scan seams
@pytest.mark.parametrize("V,T,seed", [pytest.param(V, 2 * V + 3, V, id=str(V)) for V in (63, 64, 65, 255, 256, 257, 1025)] + [pytest.param(2049, 5, 1, id="2049-5")])
def test_sizes_around_a_wave_a_workgroup_and_a_scanned_block(V, T, seed):
    """64 cells: clusters of many members from V = 255 on, leaders and dropped triangles on both sides of every seam; T = 2 V + 3 differs from V.  The last
    case has more workgroups of vertices (three) than of triangles (one): the scan's words are sized by the larger, each pass is launched over its own"""
    v, t, g = K.random_mesh(V, T, n=4, seed=seed)
    ref = K.cluster(v, t, g)
    assert 0 < len(ref["leader"]) <= 64 and 0 < len(ref["triangles"]) < len(t)
    _same(_cluster(v, t, g), ref)
    counts, raw = _raw(v, t, g)
    assert counts == (len(ref["leader"]), len(ref["triangles"]), 0, 0)
    _same(raw, ref)


# ---------------------------------------------------------------------------------------------------- contention, long keys, the leader
def test_seventy_thousand_vertices_in_one_cell():
    v, t, g = K.one_cell(70000)
    ref = K.cluster(v, t, g)
    assert len(ref["leader"]) == 1 and ref["members"].tolist() == [70000] and len(ref["triangles"]) == 0
    valid, cell, q, key = K.cells(v, g)
    assert q.sum(axis=0).min() > 2 ** 44                                                 # the sums are not 32-bit
    _same(_cluster(v, t, g), ref)


def test_keys_beyond_32_bits():
    v, t, g = K.far_cells(4096, 3)
    valid, cell, q, key = K.cells(v, g)
    assert valid.all() and key.min() >= 2 ** 61 and len(np.unique(key)) == 4096
    ref = K.cluster(v, t, g)
    assert len(ref["leader"]) == 4096 and (ref["members"] == 3).all() and len(ref["triangles"]) > len(t) // 2
    _same(_cluster(v, t, g), ref)
    # cells that agree in the low 32 bits of the key and differ above them: half as many clusters if the compare-exchange looked at 32 bits
    twins = np.stack([np.stack([np.full(8, c), np.arange(8) // 4, np.arange(8) % 4], axis=1) for c in (2 ** 20, 2 ** 20 + 2 ** 10)]).reshape(-1, 3) + 0.5
    g2 = K.grid(0.0, 1.0, [2 ** 21, 2 ** 11, 2 ** 21])                                   # key = (cx 2^11 + cy) 2^21 + cz: cx moves bits 32 and up only
    r = _cluster(twins, K.strip_triangles(16), g2)
    _same(r, K.cluster(twins, K.strip_triangles(16), g2))
    assert len(r["leader"]) == 16


def test_the_leader_is_the_smallest_id_not_the_first_arrival():
    """the floater mesh with its vertex ids under a seeded permutation: the same cells merge, each numbered by its smallest NEW id, and the integer sums do not
    depend on the order of the adds -- the set of positions is the same bit for bit"""
    v, t, shape, kw = _mc_case("floaters")
    g = K.mc_grid(shape, 2)
    plain = _cluster(v, t, g)
    pv, pt = K.permuted(v, t)
    ref = K.cluster(pv, pt, g)
    got = _cluster(pv, pt, g)
    _same(got, ref)
    assert not np.array_equal(got["leader"], plain["leader"]) and len(got["leader"]) == len(plain["leader"]) and len(got["triangles"]) == len(plain["triangles"])
    rows = lambda p: p[np.lexsort(p.T[::-1])]
    assert np.array_equal(rows(got["positions"]), rows(plain["positions"]))
    assert np.array_equal(np.sort(got["members"]), np.sort(plain["members"]))


def test_clusters_do_not_depend_on_the_run_or_the_triangle_order():
    v, t, shape, kw = _mc_case("noise_iso0")
    g = K.mc_grid(shape, 2)
    a, b = _cluster(v, t, g), _cluster(v, t, g)
    _same(b, a)
    p = np.random.RandomState(11).permutation(len(t))
    c, d = _cluster(v, t[p], g), _cluster(v, t[p], g)
    _same(d, c)
    for k in ("cluster", "leader", "members", "positions"):
        assert c[k].tobytes() == a[k].tobytes(), k                                      # the clusters are the vertices' alone
    _same(c, K.cluster(v, t[p], g))
    assert np.array_equal(np.sort(p[c["kept_triangles"]]), a["kept_triangles"])


# ---------------------------------------------------------------------------------------------------- marching-cubes meshes
@pytest.mark.parametrize("k", [1, 1.5, 2, 4])
@pytest.mark.parametrize("name", ["noise_iso0", "open_noise", "floaters"])
def test_marching_cubes_meshes(name, k):
    v, t, shape, kw = _mc_case(name)
    g = K.mc_grid(shape, k, **kw)
    ref = K.cluster(v, t, g)
    assert ref["bad_vertices"] == 0 and ref["bad_triangles"] == 0 and 0 < len(ref["leader"]) < len(v) and 0 < len(ref["triangles"]) < len(t)      # no case passes vacuously
    got = _cluster(v, t, g)
    _same(got, ref)
    if name == "floaters":                                                              # a closed oriented mesh: the edge balance survives (tests/test_mesh_decimate_host.py)
        fwd, fc, rev, rc = K.edge_balance(got["triangles"])
        assert np.array_equal(fwd, rev) and np.array_equal(fc, rc)


# ---------------------------------------------------------------------------------------------------- invalid vertices and triangles
def test_invalid_vertices_and_triangles_are_counted_and_never_emitted():
    from avatarcraft_amd import mesh_decimate
    v, t, shape, kw = _mc_case("floaters")
    g = K.mc_grid(shape, 2)
    V = len(v)
    v = v.copy()
    hi = g["h"] * g["n"][0]
    for i, bad in zip((0, 5, 300, 301, V - 1, 1000), ([np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [-1e-9, 1.0, 1.0], [1.0, 1.0, hi + g["h"]], [1.0, -np.inf, 1.0], [np.nan] * 3)):
        v[i] = bad
    v[7] = [hi, hi, hi + 0.5 * g["h"]]                                                   # inside the slack of one cell: valid, in the last cell
    extra = np.array([[-1, 1, 2], [3, V, 4], [6, 8, -2147483648], [2147483647, 9, 10], [V - 2, V - 3, V]], np.int32)      # five with an index outside [0, V)
    mixed = np.concatenate([t[:100], extra, t[100:]]).astype(np.int32)
    ref = K.cluster(v, mixed, g)
    assert ref["bad_vertices"] == 6 and ref["bad_triangles"] > 5 + 6 and ref["cluster"][7] >= 0 and (ref["cluster"][[0, 5, 300, 301, V - 1, 1000]] == -1).all()
    counts, raw = _raw(v, mixed, g)
    assert counts == (len(ref["leader"]), len(ref["triangles"]), ref["bad_vertices"], ref["bad_triangles"])
    _same(raw, ref)                                                                     # labelled and emitted as if the invalid ones were absent
    assert (raw["triangles"] >= 0).all() and not np.isin(raw["kept_triangles"], np.arange(100, 105)).any()
    with pytest.raises(RuntimeError, match=r"6 of %d vertices .* %d of %d triangles" % (V, ref["bad_triangles"], len(mixed))):
        mesh_decimate.mesh_cluster(_dev(v, torch.float64), _dev(mixed, torch.int32), g)
    with pytest.raises(RuntimeError, match=r"0 of %d vertices .* 5 of %d triangles" % (V, len(mixed))):
        mesh_decimate.mesh_cluster(_dev(_mc_case("floaters")[0], torch.float64), _dev(mixed, torch.int32), g)
    with pytest.raises(RuntimeError, match="mesh_cluster"):
        mesh_decimate.decimate_mesh(dict(vertices=_dev(v, torch.float64), triangles=_dev(mixed, torch.int32)), g)
    counts, raw = _raw(np.zeros((0, 3)), [[0, 1, 2], [0, 0, 0]], g)                       # triangles over no vertex: all invalid
    assert counts == (0, 0, 0, 2)


def test_every_entry_refuses_before_any_launch():
    from tests.test_mesh_decimate_host import check_refusals
    assert check_refusals() == 37
    torch.cuda.synchronize()                                                            # (nothing was launched: nothing can have gone wrong on the device)


# ---------------------------------------------------------------------------------------------------- model level
THRESHOLD, RES, BOUND, KD = 0.0, 48, 1.6, 3
ATTR_KEYS = ("vertices", "normals", "colors", "sdf", "status")


def _equal(a, b, keys):
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _shade(net, v, max_move):
    from avatarcraft_amd import nsr_ops
    with torch.no_grad():
        a = nsr_ops.mesh_vertex_attrs(net._field(), v, BOUND, nsr_ops.FD_STEP, refine_steps=3, tol=1e-5, max_move=max_move, target_sdf=-THRESHOLD, want_rgb=True)
    return dict(vertices=a["positions"].double(), normals=a["normals"], colors=a["rgb"], sdf=a["sdf"], status=a["status"])


@pytest.fixture(scope="module")
def plain(rough_net):
    v, t = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True)
    return v, t, rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True)


def test_decimate_none_is_what_it_was(rough_net, plain):
    v, t, full = plain
    assert set(full) == {"vertices", "triangles", "normals", "colors", "sdf", "status"}                       # exactly today's keys
    again = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=None)
    assert set(again) == set(full)
    _equal(again, full, full)
    _equal(_shade(rough_net, v, 2.0 * BOUND / (RES - 1.0)), full, ATTR_KEYS)                                   # the projection limit is still one grid cell
    vn, tn = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=None)
    assert torch.equal(tn, t) and torch.equal(vn.view(torch.int64), v.view(torch.int64))
    tex = rough_net.extract_textured_mesh(BOUND, RES, texture_size=512, threshold=THRESHOLD, return_torch=True, decimate=None)
    assert set(tex) == set(full) | {"texture", "owner", "texel_sdf", "texel_status", "uv"}
    _equal(tex, full, full)


def test_colored_mesh_is_decimate_then_shade_by_hand(rough_net, plain):
    from avatarcraft_amd.mesh_decimate import cluster_grid, decimate_mesh
    v, t, full = plain
    g = cluster_grid(BOUND, RES, KD)
    dm = decimate_mesh(dict(vertices=v, triangles=t), g)
    assert set(dm) == {"vertices", "triangles", "cluster", "cluster_members"}
    ref = K.cluster(v.cpu().numpy(), t.cpu().numpy(), g)
    assert 0 < len(ref["leader"]) < v.shape[0] // 4 and 0 < len(ref["triangles"]) < t.shape[0] // 4
    for k, kk in (("vertices", "positions"), ("triangles", "triangles"), ("cluster", "cluster"), ("cluster_members", "members")):
        assert dm[k].cpu().numpy().tobytes() == ref[kk].tobytes(), k
    got = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
    assert set(got) == set(full) | {"cluster_members"}
    want = _shade(rough_net, dm["vertices"], g["h"])                                                           # never further than one CLUSTER cell
    _equal(got, want, ATTR_KEYS)
    assert torch.equal(got["triangles"], dm["triangles"]) and torch.equal(got["cluster_members"], dm["cluster_members"])
    vg, tg = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)       # no field pass: the cluster means, unprojected
    assert torch.equal(tg, dm["triangles"]) and torch.equal(vg.view(torch.int64), dm["vertices"].view(torch.int64))
    as_numpy = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, decimate=KD)
    assert all(isinstance(x, np.ndarray) for x in as_numpy.values()) and as_numpy["cluster_members"].tobytes() == ref["members"].tobytes()
    with pytest.raises(RuntimeError, match="decimate"):
        rough_net.extract_geometry(BOUND, 32, mesher="tetra", decimate=KD)
    with pytest.raises(ValueError, match="cluster_grid: k"):
        rough_net.extract_geometry(BOUND, 32, decimate=0.5)
    with pytest.raises(RuntimeError, match="per-vertex entries"):
        decimate_mesh(full, g)                                                         # shaded meshes are decimated before the shading, never after


def test_dense_equals_streamed(rough_net):
    vd, td = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
    vs, ts = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD, slab_layers=16)
    assert td.shape[0] > 0 and torch.equal(td, ts) and torch.equal(vd.view(torch.int64), vs.view(torch.int64))
    a = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
    b = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD, slab_layers=16)
    assert set(a) == set(b)
    _equal(a, b, a)


def test_components_then_decimate_in_that_order(rough_net, plain):
    from avatarcraft_amd.geometry import clean_mesh
    from avatarcraft_amd.mesh_decimate import cluster_grid, decimate_mesh
    v, t, full = plain
    g = cluster_grid(BOUND, RES, KD)
    cleaned = clean_mesh(dict(vertices=v, triangles=t), "largest")
    assert 0 < cleaned["triangles"].shape[0] < t.shape[0]                               # the rough field has floaters at this resolution
    dm = decimate_mesh(cleaned, g)
    assert set(dm) == {"vertices", "triangles", "cluster", "cluster_members", "component_sizes", "components_kept"}
    other = decimate_mesh(dict(vertices=v, triangles=t), g)
    assert other["vertices"].shape[0] > dm["vertices"].shape[0]                          # (the other order, or no cleaning, keeps the floaters' clusters)
    vg, tg = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, components="largest", decimate=KD)
    assert torch.equal(tg, dm["triangles"]) and torch.equal(vg.view(torch.int64), dm["vertices"].view(torch.int64))
    got = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, components="largest", decimate=KD)
    assert set(got) == set(full) | {"cluster_members", "component_sizes", "components_kept"}
    _equal(got, _shade(rough_net, dm["vertices"], g["h"]), ATTR_KEYS)
    _equal(got, dm, ("triangles", "cluster_members", "component_sizes", "components_kept"))


def test_textured_mesh_lays_the_atlas_out_for_the_decimated_triangles(rough_net, plain):
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.geometry import atlas_layout
    from avatarcraft_amd.mesh_decimate import cluster_grid, decimate_mesh
    v, t, full = plain
    g = cluster_grid(BOUND, RES, KD)
    got = rough_net.extract_textured_mesh(BOUND, RES, texture_size=512, threshold=THRESHOLD, return_torch=True, decimate=KD)
    col = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
    assert set(got) == set(col) | {"texture", "owner", "texel_sdf", "texel_status", "uv"}
    _equal(got, col, col)
    n = got["triangles"].shape[0]
    lay, lay_all = atlas_layout(n, 512), atlas_layout(t.shape[0], 512)
    assert 0 < n < t.shape[0] and int(got["owner"].max()) == n - 1
    assert np.array_equal(got["uv"].cpu().numpy(), lay["uv"]) and lay["cell"] > lay_all["cell"]                 # fewer triangles: larger cells
    with torch.no_grad():
        b = nsr_ops.mesh_bake_texture(rough_net._field(), got["vertices"].float(), got["triangles"], 512, lay["cell"], BOUND, nsr_ops.FD_STEP, refine_steps=3, tol=1e-5,
                                      max_move=g["h"], target_sdf=-THRESHOLD)
    assert torch.equal(b["owner"], got["owner"]) and torch.equal(b["status"], got["texel_status"]) and torch.equal(b["sdf"].view(torch.int32), got["texel_sdf"].view(torch.int32))
    with pytest.raises(RuntimeError, match="textured mesh"):
        decimate_mesh(got, g)                                                          # decimated before the bake, never after
