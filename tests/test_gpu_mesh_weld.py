"""-m gpu: welding the decimated mesh and reporting its topology on the device -- ac_mesh_weld_count / _emit and ac_mesh_topology (csrc/mesh_weld.hip) through the
raw entries, mesh_weld.mesh_weld / mesh_topology / weld_mesh, NeRFNetwork.export_weld and weld= of drivers.export_mesh -- against the numpy restatement of
tests/mesh_weld_cases.py (which tests/test_mesh_weld_host.py checks against hand-worked index buffers).  Everything compared is an integer: every comparison is
exact equality.  The shapes are the smallest at which the kernels can go wrong: the sizes around a wave, a workgroup and the 1024 items of a scanned workgroup,
one slot that every claim and every add contends on, indices and edge keys beyond 16 and 32 bits, the triangle order under a permutation, real marching-cubes
meshes decimated on the device.  (mesh_cluster.hip after the move of its key claim into mesh_index.hpp: tests/test_gpu_mesh_decimate.py, untouched.)"""
import numpy as np
import pytest
import torch

from tests import mesh_decimate_cases as K
from tests import mesh_weld_cases as W
from tests.test_gpu_mesh_components import rough_net                                    # noqa: F401 (the fixture: the small network with the rough table)
from tests.test_gpu_mesh_decimate import ATTR_KEYS, BOUND, RES, THRESHOLD, _equal, _mc_case, _shade
from tests.test_gpu_model import DEV

pytestmark = pytest.mark.gpu
KEYS = ("vertex_map", "kept_vertices", "triangles", "kept_triangles")


def _dev(t):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(t).reshape(-1, 3))).to(device=DEV, dtype=torch.int32).contiguous()


def _weld(t, V):
    """mesh_weld.mesh_weld -> numpy"""
    from avatarcraft_amd import mesh_weld
    r = mesh_weld.mesh_weld(_dev(t), V)
    assert set(r) == set(KEYS) | {"report"} and all(r[k].is_cuda for k in KEYS) and tuple(r["report"]) == W.REPORT_KEYS
    return {k: (x.cpu().numpy() if k in KEYS else x) for k, x in r.items()}


def _topology(t, V):
    from avatarcraft_amd import mesh_weld
    r = mesh_weld.mesh_topology(_dev(t), V)
    assert all(type(x) is int for k, x in r.items() if k != "closed_manifold") and type(r["closed_manifold"]) is bool
    return r


def _same(got, ref):
    assert got["report"] == ref["report"]
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), k


def _raw(t, V, slack=3):
    """the raw entries with outputs `slack` rows longer than needed and poisoned: -> (weld counts [8], outputs as numpy, topology counts [8])"""
    from avatarcraft_amd import _lib as L
    t = _dev(t)
    T = t.shape[0]
    lib, st = L.lib(), L.current_stream(torch.device(DEV))
    need = int(lib.ac_mesh_weld_scratch(V, T))
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    counts = torch.full((8 + slack,), -7, dtype=torch.int32, device=DEV)
    head = (t.data_ptr() if T else None, T, V, scratch.data_ptr(), need)
    assert lib.ac_mesh_weld_count(*head, counts.data_ptr(), st) == 0, lib.ac_last_error()
    c = counts.tolist()
    assert c[8:] == [-7] * slack and c[7] == 0
    nv, nt = c[0], c[1]
    full = dict(vertex_map=torch.full((V + slack,), -7, dtype=torch.int32, device=DEV), kept_vertices=torch.full((nv + slack,), -7, dtype=torch.int32, device=DEV),
                triangles=torch.full((nt + slack, 3), -7, dtype=torch.int32, device=DEV), kept_triangles=torch.full((nt + slack,), -7, dtype=torch.int32, device=DEV))
    assert lib.ac_mesh_weld_emit(*head, *(full[k].data_ptr() for k in ("vertex_map", "kept_vertices")), nv, full["triangles"].data_ptr(),
                                 full["kept_triangles"].data_ptr(), nt, st) == 0, lib.ac_last_error()
    need_t = int(lib.ac_mesh_topology_scratch(V, T))
    scratch_t = torch.empty(max(need_t, 1), dtype=torch.uint8, device=DEV)
    tc = torch.full((8 + slack,), -7, dtype=torch.int32, device=DEV)
    assert lib.ac_mesh_topology(t.data_ptr() if T else None, T, V, scratch_t.data_ptr(), need_t, tc.data_ptr(), st) == 0, lib.ac_last_error()
    torch.cuda.synchronize()
    assert tc.tolist()[8:] == [-7] * slack
    full = {k: x.cpu().numpy() for k, x in full.items()}
    n = dict(vertex_map=V, kept_vertices=nv, triangles=nt, kept_triangles=nt)
    for k, x in full.items():
        assert (x[n[k]:] == -7).all(), k                                                # nothing is written past the counts
    out = {k: x[:n[k]] for k, x in full.items()}
    out["report"] = dict(zip(W.REPORT_KEYS, c[:7]))
    return c[:8], out, tc.tolist()[:8]


def _check(t, V, raw=True):
    """weld and topology of (t, V) through Python (and the raw entries) against the restatement -> (weld reference, topology reference)"""
    ref, top = W.weld(t, V), W.topology(t, V)
    if ref["report"]["invalid"] == 0:
        _same(_weld(t, V), ref)
    assert _topology(t, V) == top
    if raw:
        counts, out, tcounts = _raw(t, V)
        _same(out, ref)
        assert tcounts == [top[k] for k in W.TOPOLOGY_KEYS]
    return ref, top


# ---------------------------------------------------------------------------------------------------- degenerate sizes
def test_nothing_and_one_triangle():
    none = np.zeros((0, 3), np.int32)
    r = _weld(none, 0)                                                                   # V = T = 0: legal, nothing is launched
    assert all(r[k].size == 0 for k in KEYS) and r["triangles"].shape == (0, 3) and r["report"] == dict.fromkeys(W.REPORT_KEYS, 0)
    counts, out, tcounts = _raw(none, 0)
    assert counts == [0] * 8 and tcounts == [0] * 8
    assert _topology(none, 0) == W.topology(none, 0)
    ref, top = _check([[0, 1, 2]], 3)
    assert ref["report"]["triangles"] == 1 and (top["edges"], top["boundary"]) == (3, 3)
    ref, top = _check([[4, 2, 2]], 5)                                                    # one degenerate triangle: nothing is kept
    assert ref["report"]["degenerate"] == 1 and ref["report"]["vertices"] == 0 and top["edges"] == 0
    ref, top = _check(none, 5)                                                           # vertices and no triangle: every vertex is an orphan
    assert ref["vertex_map"].tolist() == [-1] * 5 and top["referenced"] == 0


# ---------------------------------------------------------------------------------------------------- the scan seams
@pytest.mark.parametrize("V", [12, 5000])
@pytest.mark.parametrize("T", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_sizes_around_a_wave_a_workgroup_and_a_scanned_block(T, V):
    """V = 12: at most 220 vertex sets, so from T = 255 on groups of many members of both signs, cancelling and repeating ones and degenerate triangles on both
    sides of every seam.  V = 5000: five scanned workgroups of vertices over at most three of triangles -- the scan's words are sized by the larger, each pass
    is launched over its own -- and most vertices are orphans; a third of the triangles repeat or reverse another one"""
    t = W.random_triangles(V, T, seed=T) if V == 12 else W.sparse_triangles(V, T, seed=T)
    ref, top = _check(t, V)
    rep = ref["report"]
    assert 0 < rep["triangles"] < T and rep["cancelled"] > 0 and rep["repeated"] > 0                        # no case passes vacuously
    if V == 12:
        assert rep["degenerate"] > 0 and rep["excess"] > 0 and top["nonmanifold"] > 0
    if V == 5000:
        assert 0 < rep["vertices"] < V and top["boundary"] > 0 and top["misoriented"] > 0


# ---------------------------------------------------------------------------------------------------- contention, long keys, the order
@pytest.mark.parametrize("n_plus,n_minus,kept", [(35000, 35000, 0), (35001, 35000, 1), (34999, 35002, 1)])
def test_seventy_thousand_copies_of_one_vertex_set(n_plus, n_minus, kept):
    """every claim, both mins and both adds of the mesh land on one slot; net = 0, +1 and -3"""
    t = W.one_set(n_plus, n_minus)
    ref, top = _check(t, 8, raw=False)
    rep = ref["report"]
    assert rep["triangles"] == kept and rep["excess"] == max(abs(n_plus - n_minus) - 1, 0)
    assert rep["cancelled"] == (0 if kept else n_plus + n_minus) and rep["repeated"] == (n_plus + n_minus - 1 if kept else 0)
    assert (top["edges"], top["nonmanifold"], top["faces"]) == (3, 3, n_plus + n_minus)
    if kept:                                                                            # the smallest member of the majority sign, whoever claimed the slot
        majority = W.signs(t.astype(np.int64)) == (n_plus > n_minus)
        assert ref["kept_triangles"].tolist() == [int(np.flatnonzero(majority)[0])]


def test_indices_beyond_16_bits_and_edge_keys_beyond_32():
    t, V = W.high_indices()
    assert t.min() > 2 ** 16
    ref, top = _check(t, V)
    assert ref["report"]["cancelled"] > 0 and ref["report"]["repeated"] > 0 and ref["report"]["vertices"] == 40 and top["edges"] == 780
    t, V = W.low_word_twins()                                                           # edges that agree in the low 32 bits of their key
    ref, top = _check(t, V)
    assert top["edges"] == 9 and ref["report"]["triangles"] == 7


def test_the_survivor_is_the_smallest_index_not_the_first_arrival():
    """the triangle order under a seeded permutation: the same vertex sets survive with the same orientation, each as the smallest NEW index of its majority sign"""
    for t, V in ((W.random_triangles(12, 2049, seed=2049), 12), W.high_indices()):
        plain = _weld(t, V)
        pt, p = W.permuted_triangles(t)
        got, ref = _weld(pt, V), W.weld(pt, V)
        _same(got, ref)
        assert not np.array_equal(p[got["kept_triangles"]], plain["kept_triangles"])      # other members survive ...
        a, b = t[plain["kept_triangles"]].astype(np.int64), pt[got["kept_triangles"]].astype(np.int64)
        assert W.vertex_sets(a) == W.vertex_sets(b)                                      # ... of the same groups ...
        order = lambda m: np.lexsort(np.sort(m, axis=1).T[::-1])
        assert np.array_equal(W.signs(a)[order(a)], W.signs(b)[order(b)])                # ... with the same orientation
        assert np.array_equal(got["vertex_map"], plain["vertex_map"]) and _topology(pt, V) == _topology(t, V)


def test_two_runs_are_identical():
    m, V = _decimated("floaters", 5)
    a, b = _weld(m, V), _weld(m, V)
    _same(b, a)
    assert _topology(m, V) == _topology(m, V)
    t = W.random_triangles(12, 2049, seed=5)
    _same(_weld(t, 12), _weld(t, 12))


# ---------------------------------------------------------------------------------------------------- marching-cubes meshes, decimated on the device
def _decimated(name, k):
    """the triangles of a marching-cubes case after mesh_decimate.mesh_cluster on the device -> (triangles [T,3] int32 numpy, V)"""
    from avatarcraft_amd import mesh_decimate
    v, t, shape, kw = _mc_case(name)
    r = mesh_decimate.mesh_cluster(torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV), K.mc_grid(shape, k, **kw))
    return r["triangles"].cpu().numpy(), int(r["leader"].shape[0])


@pytest.mark.parametrize("name,k", [("floaters", 3), ("floaters", 5), ("noise_iso0", 2), ("noise_iso0", 3), ("open_noise", 2)])
def test_decimated_marching_cubes_meshes(name, k):
    m, V = _decimated(name, k)
    ref, top = _check(m, V)
    rep = ref["report"]
    assert rep["invalid"] == 0 and rep["degenerate"] == 0 and 0 < rep["triangles"] <= len(m)
    after = _topology(ref["triangles"], rep["vertices"])
    assert after == W.topology(ref["triangles"], rep["vertices"]) and after["referenced"] == rep["vertices"] and after["faces"] == rep["triangles"]
    if name == "open_noise":
        assert top["boundary"] > 0 and not top["closed_manifold"]                        # an open surface: the report says so
    assert rep["vertices"] < V or rep["triangles"] < len(m)                               # no case passes vacuously: there is something to weld
    if name == "noise_iso0":                                                            # noise collapses onto itself everywhere: every kind of group
        assert rep["cancelled"] > 0 and rep["repeated"] > 0 and rep["excess"] > 0 and top["nonmanifold"] > 0
    if name == "floaters":                                                              # a closed oriented mesh: after the weld it is a closed manifold (again)
        assert rep["excess"] == 0 and after["closed_manifold"]
        fwd, fc, rev, rc = K.edge_balance(ref["triangles"])
        assert np.array_equal(fwd, rev) and np.array_equal(fc, rc)
        if k == 5:                                                                      # in this grid k = 3 leaves orphan vertices only; k = 5 a back-to-back pair
            assert rep["cancelled"] > 0 and not top["closed_manifold"]


# ---------------------------------------------------------------------------------------------------- invalid triangles, refusals
def test_invalid_triangles_are_counted_and_never_emitted():
    from avatarcraft_amd import mesh_weld
    m, V = _decimated("floaters", 5)
    extra = np.array([[-1, 1, 2], [3, V, 4], [6, 8, -2147483648], [2147483647, 9, 10], [V - 2, V - 3, V]], np.int32)
    mixed = np.concatenate([m[:100], extra, m[100:]]).astype(np.int32)
    ref, top = W.weld(mixed, V), W.topology(mixed, V)
    assert ref["report"]["invalid"] == 5 and top["invalid"] == 5
    counts, out, tcounts = _raw(mixed, V)
    _same(out, ref)
    assert tcounts == [top[k] for k in W.TOPOLOGY_KEYS] and not np.isin(out["kept_triangles"], np.arange(100, 105)).any()
    assert _topology(mixed, V) == top
    with pytest.raises(RuntimeError, match=r"mesh_weld: 5 of %d triangles name an index outside \[0, %d\)" % (len(mixed), V)):
        mesh_weld.mesh_weld(_dev(mixed), V)
    with pytest.raises(RuntimeError, match="triangles over no vertex"):
        mesh_weld.mesh_weld(_dev(m), 0)


def test_every_entry_refuses_before_any_launch():
    from tests.test_mesh_weld_host import check_refusals
    assert check_refusals() == 26
    torch.cuda.synchronize()                                                            # (nothing was launched: nothing can have gone wrong on the device)


# ---------------------------------------------------------------------------------------------------- model level
KD = 3


class _welding:
    """net.export_weld = True inside the block"""
    def __init__(self, net):
        self.net = net

    def __enter__(self):
        self.net.export_weld = True

    def __exit__(self, *exc):
        del self.net.export_weld


@pytest.fixture(scope="module")
def by_hand(rough_net):
    """the export's steps one by one: geometry -> decimate_mesh -> weld_mesh, and the decimated mesh shaded without a weld"""
    from avatarcraft_amd.mesh_decimate import cluster_grid, decimate_mesh
    from avatarcraft_amd.mesh_weld import weld_mesh
    assert rough_net.export_weld is False
    v, t = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True)
    g = cluster_grid(BOUND, RES, KD)
    dm = decimate_mesh(dict(vertices=v, triangles=t), g)
    return g, dm, weld_mesh(dm)


def test_switch_off_is_what_it_was(rough_net, by_hand):
    g, dm, wm = by_hand
    got = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
    assert set(got) == {"vertices", "triangles", "normals", "colors", "sdf", "status", "cluster_members"}      # exactly today's keys: no report
    _equal(got, _shade(rough_net, dm["vertices"], g["h"]), ATTR_KEYS)                                          # decimate -> shade, nothing in between
    assert torch.equal(got["triangles"], dm["triangles"]) and torch.equal(got["cluster_members"], dm["cluster_members"])
    vg, tg = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
    assert torch.equal(tg, dm["triangles"]) and torch.equal(vg.view(torch.int64), dm["vertices"].view(torch.int64))


def test_weld_mesh_is_the_restatement_gathered(by_hand):
    from avatarcraft_amd.mesh_weld import weld_mesh
    g, dm, wm = by_hand
    V = dm["vertices"].shape[0]
    ref = W.weld(dm["triangles"].cpu().numpy(), V)
    assert set(wm) == {"vertices", "triangles", "cluster", "cluster_members", "weld"} and wm["weld"] == ref["report"]
    assert ref["report"]["vertices"] < V or ref["report"]["triangles"] < dm["triangles"].shape[0]               # there is something to weld
    assert np.array_equal(wm["triangles"].cpu().numpy(), ref["triangles"])
    assert wm["vertices"].cpu().numpy().tobytes() == dm["vertices"].cpu().numpy()[ref["kept_vertices"]].tobytes()
    assert np.array_equal(wm["cluster_members"].cpu().numpy(), dm["cluster_members"].cpu().numpy()[ref["kept_vertices"]])
    c = dm["cluster"].cpu().numpy()
    assert (c >= 0).all() and np.array_equal(wm["cluster"].cpu().numpy(), ref["vertex_map"][c]) and wm["cluster"].dtype == torch.int32
    extra = dict(dm, normals=torch.arange(3 * V, device=DEV, dtype=torch.float32).reshape(V, 3), component_sizes=torch.zeros((V, 2), dtype=torch.int64, device=DEV))
    again = weld_mesh(extra)
    assert torch.equal(again["normals"], extra["normals"][torch.from_numpy(ref["kept_vertices"]).long().to(DEV)])  # per vertex: gathered
    assert again["component_sizes"] is extra["component_sizes"]                                                # not per vertex, whatever its length: carried over


def test_switch_on_is_decimate_weld_shade_by_hand(rough_net, by_hand):
    g, dm, wm = by_hand
    with _welding(rough_net):
        got = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
        vg, tg = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD)
        as_numpy = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, decimate=KD)
        streamed = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, decimate=KD, slab_layers=16)
        with pytest.raises(RuntimeError, match="export_weld"):
            rough_net.extract_geometry(BOUND, 32, mesher="tetra")
    assert rough_net.export_weld is False
    assert set(got) == {"vertices", "triangles", "normals", "colors", "sdf", "status", "cluster_members", "weld"} and got["weld"] == wm["weld"]
    _equal(got, _shade(rough_net, wm["vertices"], g["h"]), ATTR_KEYS)                                          # orphan vertices are never shaded
    assert torch.equal(got["triangles"], wm["triangles"]) and torch.equal(got["cluster_members"], wm["cluster_members"])
    assert torch.equal(tg, wm["triangles"]) and torch.equal(vg.view(torch.int64), wm["vertices"].view(torch.int64))
    assert as_numpy["weld"] == wm["weld"] and all(isinstance(x, np.ndarray) for k, x in as_numpy.items() if k != "weld")
    assert as_numpy["triangles"].tobytes() == wm["triangles"].cpu().numpy().tobytes()
    assert set(streamed) == set(got) and streamed["weld"] == got["weld"]                                        # the dense and the streamed route agree
    _equal(streamed, got, [k for k in got if k != "weld"])


def test_weld_without_decimation_and_after_the_cleaning(rough_net):
    from avatarcraft_amd.geometry import clean_mesh
    from avatarcraft_amd.mesh_weld import weld_mesh
    v, t = rough_net.extract_geometry(BOUND, RES, threshold=THRESHOLD, return_torch=True)
    cleaned = clean_mesh(dict(vertices=v, triangles=t), "largest")
    want = weld_mesh(cleaned)
    assert set(want) == {"vertices", "triangles", "component_sizes", "components_kept", "weld"}
    assert want["weld"]["triangles"] == cleaned["triangles"].shape[0] and want["weld"]["cancelled"] == 0        # a marching-cubes mesh has nothing to weld
    with _welding(rough_net):
        got = rough_net.extract_colored_mesh(BOUND, RES, threshold=THRESHOLD, return_torch=True, components="largest")
    assert got["weld"] == want["weld"] and "cluster_members" not in got
    _equal(got, want, ("triangles", "component_sizes", "components_kept"))
    _equal(got, _shade(rough_net, want["vertices"], 2.0 * BOUND / (RES - 1.0)), ATTR_KEYS)


def test_textured_mesh_lays_the_atlas_out_for_the_welded_triangles(rough_net, by_hand):
    from avatarcraft_amd.geometry import atlas_layout
    from avatarcraft_amd.mesh_weld import weld_mesh
    g, dm, wm = by_hand
    with _welding(rough_net):
        got = rough_net.extract_textured_mesh(BOUND, RES, texture_size=512, threshold=THRESHOLD, return_torch=True, decimate=KD)
    n = wm["weld"]["triangles"]
    assert got["triangles"].shape[0] == n and torch.equal(got["triangles"], wm["triangles"]) and got["weld"] == wm["weld"]
    assert np.array_equal(got["uv"].cpu().numpy(), atlas_layout(n, 512)["uv"]) and int(got["owner"].max()) == n - 1
    with pytest.raises(RuntimeError, match="textured mesh"):
        weld_mesh(got)                                                                 # welded before the bake, never after


def test_the_driver_writes_the_welded_mesh_and_reports_its_topology(rough_net, by_hand, tmp_path):
    from avatarcraft_amd import drivers
    from tests.test_mesh_export_host import read_ply
    g, dm, wm = by_hand
    path = str(tmp_path / "welded.ply")
    mesh = drivers.export_mesh(rough_net, path, bound=BOUND, resolution=RES, threshold=THRESHOLD, decimate=KD, weld=True)
    assert rough_net.export_weld is False
    props, table, faces, size = read_ply(path)
    tris = wm["triangles"].cpu().numpy()
    assert len(faces) == wm["weld"]["triangles"] and len(table) == wm["weld"]["vertices"] and np.array_equal(np.asarray(faces), tris)
    assert mesh["weld"] == wm["weld"] and mesh["topology"] == W.topology(tris, wm["weld"]["vertices"])
    assert mesh["topology"]["faces"] == len(faces) and mesh["topology"]["referenced"] == len(table)
    plain = drivers.export_mesh(rough_net, str(tmp_path / "plain.ply"), bound=BOUND, resolution=RES, threshold=THRESHOLD, decimate=KD)
    assert "weld" not in plain and "topology" not in plain and plain["triangles"].shape[0] == dm["triangles"].shape[0]
    obj = drivers.export_mesh(rough_net, str(tmp_path / "welded.obj"), bound=BOUND, resolution=RES, threshold=THRESHOLD, decimate=KD, weld=True, texture_size=512)
    n_faces = sum(1 for ln in open(str(tmp_path / "welded.obj")) if ln.startswith("f "))
    assert n_faces == wm["weld"]["triangles"] and obj["topology"] == mesh["topology"] and rough_net.export_weld is False
