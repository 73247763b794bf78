"""-m gpu: cleaning the exported mesh on the device -- ac_mesh_components / ac_mesh_compact_count / _emit (csrc/mesh_components.hip) through the raw entries,
nsr_ops.mesh_components / mesh_compact, geometry.clean_mesh and components= of the model's extractors -- against the numpy union-find of
tests/mesh_component_cases.py (which tests/test_mesh_components_host.py checks against scipy).  Everything compared is an integer or a gathered copy: every
comparison is exact equality.  The shapes are the smallest at which the kernels can go wrong: the sizes around a wave, a workgroup and the 1024 items of a scanned
workgroup, chains that make the deepest parent paths, one word that every hook contends on, many components, real marching-cubes meshes."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_component_cases as K
from tests.test_gpu_model import golden_net, DEV

pytestmark = pytest.mark.gpu


def _dev(a, dt=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt).contiguous()


def _label(tris, V):
    """nsr_ops.mesh_components -> numpy"""
    from avatarcraft_amd import nsr_ops
    r = nsr_ops.mesh_components(_dev(np.asarray(tris).reshape(-1, 3)), V)
    assert r["root"].is_cuda and r["component"].is_cuda and r["sizes"].is_cuda
    return dict(root=r["root"].cpu().numpy(), component=r["component"].cpu().numpy(), sizes=r["sizes"].cpu().numpy(), n_components=r["n_components"])


def _label_raw(tris, V, max_components=None):
    """the raw entry: -> (rc, dict with n_bad and the size table as allocated, rows past C poisoned with 0xffffffff)"""
    from avatarcraft_amd import _lib as L
    t = _dev(np.asarray(tris).reshape(-1, 3))
    T = t.shape[0]
    maxc = V if max_components is None else max_components
    root, comp = torch.full((V,), -7, dtype=torch.int32, device=DEV), torch.full((V,), -7, dtype=torch.int32, device=DEV)
    sizes = torch.full((max(maxc, 1), 2), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    need = int(L.lib().ac_mesh_components_scratch(V, T))
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    rc = L.lib().ac_mesh_components(t.data_ptr() if T else None, T, V, root.data_ptr(), comp.data_ptr(), sizes.data_ptr(), maxc, counts.data_ptr(), scratch.data_ptr(), need,
                                    L.current_stream(torch.device(DEV)))
    torch.cuda.synchronize()
    c, bad = counts.tolist()
    return rc, dict(root=root.cpu().numpy(), component=comp.cpu().numpy(), sizes=sizes.cpu().numpy().astype(np.int64), n_components=c, n_bad=bad)


def _same_labels(got, ref):
    assert got["n_components"] == ref["n_components"]
    assert np.array_equal(got["root"], ref["root"]) and np.array_equal(got["component"], ref["component"])
    assert np.array_equal(got["sizes"][:ref["n_components"]], ref["sizes"])


def _compact(tris, component, keep):
    from avatarcraft_amd import nsr_ops
    r = nsr_ops.mesh_compact(_dev(np.asarray(tris).reshape(-1, 3)), _dev(component), _dev(keep, torch.bool))
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same_compaction(got, ref):
    assert set(got) == {"vertex_map", "kept_vertices", "triangles", "kept_triangles"}
    for k in got:
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k


def _gpu_mc(u, iso, **kw):
    from avatarcraft_amd import nsr_ops
    v, t = nsr_ops.marching_cubes(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(DEV), iso, **kw)
    return v.cpu().numpy(), t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mc_case(name):
    """(vertices, triangles, yardstick) of a marching-cubes mesh, made once: nsr_ops.marching_cubes on the device, the union-find on the host"""
    padded, (opened, kw) = K.noise_volumes()
    u, iso, kw = {"noise_iso0": (padded, 0.0, {}), "noise_iso08": (padded, 0.8, {}), "open_noise": (opened, 0.2, kw), "floaters": (K.body_with_floaters(), 0.0, {})}[name]
    v, t = _gpu_mc(u, iso, **kw)
    return v, t, K.components(t, len(v))


# ---------------------------------------------------------------------------------------------------- degenerate sizes
def test_no_triangles_no_vertices_one_two_triangles():
    r = _label(np.zeros((0, 3), np.int32), 5)                                         # T = 0: V singleton components
    assert r["n_components"] == 5 and r["root"].tolist() == list(range(5)) and r["component"].tolist() == list(range(5)) and r["sizes"].tolist() == [[1, 0]] * 5
    r = _label(np.zeros((0, 3), np.int32), 0)                                         # V = 0: C = 0, no launch
    assert r["n_components"] == 0 and r["root"].shape == (0,) and r["component"].shape == (0,) and r["sizes"].shape == (0, 2)
    rc, raw = _label_raw(np.zeros((0, 3), np.int32), 0)
    assert rc == 0 and raw["n_components"] == 0 and raw["n_bad"] == 0
    c = _compact(np.zeros((0, 3), np.int32), np.zeros(0, np.int32), np.zeros(0, bool))
    assert all(v.size == 0 for v in c.values())
    for tris, V in (([[0, 1, 2]], 3), ([[3, 1, 2]], 5),                               # one triangle; one triangle among isolated vertices
                    ([[0, 1, 2], [2, 3, 4]], 5), ([[4, 3, 2], [2, 1, 0]], 6),           # two triangles sharing one vertex
                    ([[0, 1, 2], [2, 1, 3]], 4), ([[5, 1, 2], [2, 1, 0]], 6),           # two triangles sharing an edge
                    ([[0, 1, 2], [3, 4, 5]], 6), ([[2, 2, 5], [5, 5, 5], [0, 1, 1], [0, 1, 1]], 6)):      # disjoint; degenerate and duplicate ones count and join
        tris = np.array(tris, np.int32)
        ref = K.components(tris, V)
        _same_labels(_label(tris, V), ref)
        for keep in (np.ones(ref["n_components"], bool), np.zeros(ref["n_components"], bool), np.arange(ref["n_components"]) % 2 == 0):
            _same_compaction(_compact(tris, ref["component"], keep), K.compact(tris, ref["component"], keep))
    assert _label([[0, 1, 2], [2, 1, 3]], 4)["sizes"].tolist() == [[4, 2]]


# ---------------------------------------------------------------------------------------------------- strips, fan, many components
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1023, 1025, 100000])
def test_strip_is_one_component_with_root_zero(n):
    """triangles (i, i+1, i+2): the ids ascending, descending (every hook of a wave lands on the link before it: the deepest chains) and permuted; the triangle
    order as it is and shuffled.  100 000 triangles span many workgroups and all XCDs."""
    for order in ("ascending", "descending", "permuted"):
        for shuffled in (False, True):
            tris, V = K.strip(n, order, seed=n, shuffle_triangles=shuffled)
            r = _label(tris, V)
            assert r["n_components"] == 1 and r["sizes"].tolist() == [[V, n]], (order, shuffled)
            assert not r["root"].any() and not r["component"].any(), (order, shuffled)


def test_fan_contends_on_one_word():
    """50 000 triangles (hub, 2i, 2i+1) with hub = V - 1: every hook contends on the hub's word, and the hub is never the root"""
    tris, V = K.fan(50000)
    r = _label(tris, V)
    assert r["n_components"] == 1 and r["sizes"].tolist() == [[V, 50000]] and not r["root"].any() and not r["component"].any()
    r = _label(tris[np.random.RandomState(2).permutation(len(tris))], V)
    assert r["n_components"] == 1 and r["sizes"].tolist() == [[V, 50000]] and not r["root"].any()


def test_many_components_are_ordered_by_root():
    tris, V = K.disjoint(50000)
    r = _label(tris, V)
    assert r["n_components"] == 50000 and (r["sizes"] == np.array([3, 1])).all()
    assert np.array_equal(r["root"][tris], np.repeat(tris.min(axis=1)[:, None], 3, axis=1))
    roots = np.sort(tris.min(axis=1))
    assert np.array_equal(r["component"], np.searchsorted(roots, r["root"]))           # the rank of the root among the roots, ascending
    assert np.array_equal(r["component"][roots], np.arange(50000))


# ---------------------------------------------------------------------------------------------------- marching-cubes meshes
@pytest.mark.parametrize("name,at_least", [("noise_iso0", 50), ("noise_iso08", 50), ("open_noise", 50), ("floaters", 4)])
def test_marching_cubes_meshes(name, at_least):
    """the meshes of tests/test_gpu_geometry.py's volumes and a body with floaters (on the CPU, with the oracle's mesher and scipy: 187, 775, 75 and 4 components)"""
    v, t, ref = _mc_case(name)
    assert ref["n_components"] >= at_least and ref["n_bad"] == 0                      # no case passes vacuously
    _same_labels(_label(t, len(v)), ref)
    if name == "floaters":
        from avatarcraft_amd import geometry
        assert sorted(ref["sizes"][:, 1].tolist(), reverse=True) == [3740, 224, 196, 16]
        m = geometry.clean_mesh(dict(vertices=_dev(v, torch.float64), triangles=_dev(t)), "largest")
        cv, ct = m["vertices"].cpu().numpy(), m["triangles"].cpu().numpy()
        assert len(ct) == 3740 and m["components_kept"].cpu().numpy().tolist() == (ref["sizes"][:, 1] == 3740).tolist()
        assert np.array_equal(m["component_sizes"].cpu().numpy(), ref["sizes"])
        K.mesh_checks(cv, ct)                                                          # the body alone is a closed, consistently oriented mesh that uses every vertex
        c = K.compact(t, ref["component"], ref["sizes"][:, 1] == 3740)
        assert np.array_equal(ct, c["triangles"]) and np.array_equal(cv.view(np.uint64), v[c["kept_vertices"]].view(np.uint64))


# ---------------------------------------------------------------------------------------------------- invalid, duplicate and degenerate triangles
def test_invalid_triangles_join_nothing_and_are_counted():
    from avatarcraft_amd import nsr_ops
    v, t, _ = _mc_case("floaters")
    V = len(v)
    rs = np.random.RandomState(7)
    extra = np.array([[-1, 0, 1], [5, V, 6], [7, 8, -2147483648], [V - 1, V - 1, V], [2147483647, 3, 4],        # five invalid ones (they name vertices of different components)
                      [9, 9, 10], [11, 11, 11]], np.int32)                                                     # two degenerate ones: valid
    mixed = np.concatenate([t[:100], extra, t[100:], t[:50]]).astype(np.int32)                                 # 50 duplicates
    mixed = mixed[rs.permutation(len(mixed))]
    ref = K.components(mixed, V)
    good = mixed[K.valid_triangles(mixed, V)]
    assert ref["n_bad"] == 5 and len(good) == len(mixed) - 5
    rc, raw = _label_raw(mixed, V)
    assert rc == 0 and raw["n_bad"] == 5
    _same_labels(raw, ref)
    _same_labels(raw, K.components(good, V))                                          # labelled as if the bad ones were absent
    assert (raw["sizes"][ref["n_components"]:] == -1).all()                           # rows [C, max_components) are left untouched
    with pytest.raises(RuntimeError, match="5 of %d triangles" % len(mixed)):
        nsr_ops.mesh_components(_dev(mixed), V)
    keep = np.arange(ref["n_components"]) % 2 == 1
    _same_compaction(_compact(mixed, ref["component"], keep), K.compact(mixed, ref["component"], keep))        # an invalid triangle is never emitted
    rc, short = _label_raw(t, V, max_components=2)                                    # a table that is too short: the error says so, the rest is written
    from avatarcraft_amd import _lib as L
    assert rc == 1 and "4 components, sizes holds 2 rows" in L.lib().ac_last_error().decode()
    full = K.components(t, V)
    assert short["n_components"] == 4 and np.array_equal(short["root"], full["root"]) and np.array_equal(short["component"], full["component"])
    assert np.array_equal(short["sizes"][:2], full["sizes"][:2])


# ---------------------------------------------------------------------------------------------------- determinism
def test_labels_do_not_depend_on_the_run_or_the_triangle_order():
    v, t, ref = _mc_case("noise_iso0")
    a, b = _label(t, len(v)), _label(t, len(v))
    c = _label(t[np.random.RandomState(11).permutation(len(t))], len(v))
    for other in (b, c):
        _same_labels(other, a)
    _same_labels(a, ref)


# ---------------------------------------------------------------------------------------------------- compaction
def _keeps(sizes):
    C = len(sizes)
    largest = np.zeros(C, bool)
    largest[np.argmax(sizes[:, 1])] = True
    return dict(all=np.ones(C, bool), none=np.zeros(C, bool), largest=largest, every_other=np.arange(C) % 2 == 0)


@pytest.mark.parametrize("case", ["noise_iso0", "V255", "V256", "V257", "V1025"])
def test_compaction_equals_boolean_indexing(case):
    if case.startswith("V"):
        V = int(case[1:])
        tris = K.disjoint(V // 3 - 10, seed=V)[0]                                      # disjoint triangles over the low ids and isolated vertices above them ...
        tris = np.concatenate([tris, K.strip(20, "descending")[0] + (V - 22)]).astype(np.int32)      # ... a strip over the last 22 vertices
        ref = K.components(tris, V)
    else:
        v, tris, ref = _mc_case(case)
        V = len(v)
    assert ref["n_components"] >= 50
    for name, keep in _keeps(ref["sizes"]).items():
        got, want = _compact(tris, ref["component"], keep), K.compact(tris, ref["component"], keep)
        _same_compaction(got, want)
        if name == "all":
            assert np.array_equal(got["triangles"], tris) and np.array_equal(got["kept_vertices"], np.arange(V)) and np.array_equal(got["vertex_map"], np.arange(V))
        if name == "none":                                                             # V' = T' = 0: nothing of size zero is launched, no error
            assert got["kept_vertices"].shape == (0,) and got["triangles"].shape == (0, 3) and (got["vertex_map"] == -1).all()


# ---------------------------------------------------------------------------------------------------- model level
THRESHOLD = 0.0


@pytest.fixture(scope="module")
def rough_net():
    """golden_net() with the rough=True synthetic table (synthetic.field_table: seed + 1, amplitude 0.5 on every level) in place of its smooth one: on the CPU oracle's
    64^3 grid the smooth field's mesh is ONE component at every threshold tried in [-0.1, 0.1] (21 steps), the rough one's has 16 to 117 (61 at threshold 0)."""
    from avatarcraft_amd.synthetic import make_table
    net, p = golden_net()
    table = make_table(int(p["offsets"][-1]), seed=int(p["table_seed"]) + 1, amp=0.5)
    with torch.no_grad():
        net.encoder.embeddings.copy_(torch.from_numpy(table).to(DEV))
    return net


@pytest.fixture(scope="module")
def unfiltered(rough_net):
    m = rough_net.extract_colored_mesh(1.6, 64, threshold=THRESHOLD, return_torch=True)
    t = m["triangles"].cpu().numpy()
    ref = K.components(t, m["vertices"].shape[0])
    largest = np.zeros(ref["n_components"], bool)
    largest[np.argmax(ref["sizes"][:, 1])] = True                                      # (argmax: the first of equals, the lower component id)
    return m, t, ref, largest


def test_colored_mesh_of_the_largest_component_is_the_unfiltered_one_gathered(rough_net, unfiltered):
    """uses the rough=True synthetic table (see rough_net).  The attributes are per vertex, so they cannot depend on the dropped vertices: bit for bit."""
    full, t, ref, largest = unfiltered
    assert ref["n_components"] >= 2
    assert set(full) == {"vertices", "triangles", "normals", "colors", "sdf", "status"}                        # components=None: exactly today's keys
    got = rough_net.extract_colored_mesh(1.6, 64, threshold=THRESHOLD, components="largest", return_torch=True)
    assert set(got) == set(full) | {"component_sizes", "components_kept"}
    want = K.compact(t, ref["component"], largest)
    assert 0 < len(want["kept_vertices"]) < full["vertices"].shape[0]
    assert np.array_equal(got["triangles"].cpu().numpy(), want["triangles"])
    assert np.array_equal(got["component_sizes"].cpu().numpy(), ref["sizes"]) and np.array_equal(got["components_kept"].cpu().numpy(), largest)
    for k in ("vertices", "normals", "colors", "sdf", "status"):
        a, b = got[k].cpu().numpy(), full[k].cpu().numpy()[want["kept_vertices"]]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    as_numpy = rough_net.extract_colored_mesh(1.6, 64, threshold=THRESHOLD, components=("min_faces", 20))
    assert all(isinstance(x, np.ndarray) for x in as_numpy.values()) and as_numpy["components_kept"].tolist() == (ref["sizes"][:, 1] >= 20).tolist()


def test_geometry_cleaned_streamed_equals_dense(rough_net, unfiltered):
    full, t, ref, largest = unfiltered
    plain = rough_net.extract_geometry(1.6, 64, threshold=THRESHOLD, return_torch=True)
    assert isinstance(plain, tuple) and len(plain) == 2 and np.array_equal(plain[1].cpu().numpy(), t)          # components=None: what it returns today
    for spec, keep in (("largest", largest), (("min_faces", 20), ref["sizes"][:, 1] >= 20), (np.arange(ref["n_components"]) % 3 == 0,) * 2):
        want = K.compact(t, ref["component"], keep)
        vd, td = rough_net.extract_geometry(1.6, 64, threshold=THRESHOLD, components=spec, return_torch=True)
        vs, ts = rough_net.extract_geometry(1.6, 64, threshold=THRESHOLD, components=spec, slab_layers=16, return_torch=True)
        assert torch.equal(td, ts) and torch.equal(vd.view(torch.int64), vs.view(torch.int64))
        assert np.array_equal(td.cpu().numpy(), want["triangles"])
        assert np.array_equal(vd.cpu().numpy().view(np.uint64), plain[0].cpu().numpy()[want["kept_vertices"]].view(np.uint64))
    vn, tn = rough_net.extract_geometry(1.6, 64, threshold=THRESHOLD, components="largest")
    assert isinstance(vn, np.ndarray) and np.array_equal(tn, K.compact(t, ref["component"], largest)["triangles"])
    with pytest.raises(RuntimeError, match="components"):
        rough_net.extract_geometry(1.6, 32, mesher="tetra", components="largest")
    with pytest.raises(ValueError, match="select_components"):
        rough_net.extract_geometry(1.6, 32, components="biggest")


def test_textured_mesh_lays_the_atlas_out_for_the_kept_triangles(rough_net, unfiltered):
    from avatarcraft_amd.geometry import atlas_layout, clean_mesh
    full, t, ref, largest = unfiltered
    want = K.compact(t, ref["component"], largest)
    n_kept = len(want["triangles"])
    plain = rough_net.extract_textured_mesh(1.6, 64, texture_size=512, threshold=THRESHOLD, return_torch=True)
    assert set(plain) == {"vertices", "triangles", "normals", "colors", "sdf", "status", "texture", "owner", "texel_sdf", "texel_status", "uv"}      # today's keys
    got = rough_net.extract_textured_mesh(1.6, 64, texture_size=512, threshold=THRESHOLD, components="largest", return_torch=True)
    assert set(got) == set(plain) | {"component_sizes", "components_kept"}
    assert np.array_equal(got["triangles"].cpu().numpy(), want["triangles"])
    assert int(got["owner"].max()) == n_kept - 1 and int(plain["owner"].max()) == len(t) - 1
    lay_kept, lay_all = atlas_layout(n_kept, 512), atlas_layout(len(t), 512)
    assert np.array_equal(got["uv"].cpu().numpy(), lay_kept["uv"]) and np.array_equal(plain["uv"].cpu().numpy(), lay_all["uv"])
    assert lay_kept["cell"] >= lay_all["cell"]                                         # the cell of the cleaned call is at least the unfiltered call's
    with pytest.raises(RuntimeError, match="textured mesh"):
        clean_mesh(plain, "largest")                                                   # cleaned before the bake, never after
