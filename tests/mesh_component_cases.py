"""The yardstick and the cases of the mesh-cleaning tests (ac_mesh_components / ac_mesh_compact_*, csrc/mesh_components.hip): a plain numpy union-find that
restates the definitions of include/avatarcraft_hip.h -- root = the smallest vertex of the component, component = the rank of the root, sizes, the compaction by
boolean indexing -- and the small meshes at which the kernels can go wrong.  The reference has no counterpart.  Everything compared is an integer or a gathered
copy: every comparison of these tests is exact equality.  CPU tier: tests/test_mesh_components_host.py; GPU tier: tests/test_gpu_mesh_components.py."""
import numpy as np


def valid_triangles(tris, V):
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < V)).all(axis=1)


def components(tris, V):
    """-> dict(root [V] int32, component [V] int32, sizes [C,2] int64, n_components, n_bad): a serial union-find over the valid triangles that links the larger
    root under the smaller (so a component's root is its minimum), then rank and counts"""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    ok = valid_triangles(t, V)
    tv = t[ok]
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in tv.tolist():
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    lab = np.array([find(v) for v in range(V)], dtype=np.int64).reshape(V)
    roots = np.flatnonzero(lab == np.arange(V))
    comp = np.searchsorted(roots, lab)
    sizes = np.zeros((len(roots), 2), np.int64)
    sizes[:, 0] = np.bincount(comp, minlength=len(roots))
    if len(tv):
        sizes[:, 1] = np.bincount(comp[tv[:, 0]], minlength=len(roots))
    return dict(root=lab.astype(np.int32), component=comp.astype(np.int32), sizes=sizes, n_components=len(roots), n_bad=int((~ok).sum()))


def compact(tris, component, keep):
    """-> dict(vertex_map [V], kept_vertices [V'], triangles [T',3], kept_triangles [T']), all int32: boolean indexing"""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    component, keep = np.asarray(component, dtype=np.int64), np.asarray(keep).astype(bool)
    V = len(component)
    kv = keep[component] if V else np.zeros(0, bool)
    ok = valid_triangles(t, V)
    kt = ok.copy()
    kt[ok] = kv[t[ok, 0]]
    vmap = np.full(V, -1, np.int64)
    vmap[kv] = np.arange(int(kv.sum()))
    return dict(vertex_map=vmap.astype(np.int32), kept_vertices=np.flatnonzero(kv).astype(np.int32), triangles=vmap[t[kt]].astype(np.int32).reshape(-1, 3),
                kept_triangles=np.flatnonzero(kt).astype(np.int32))


def strip(n, order="ascending", seed=0, shuffle_triangles=False):
    """n triangles (i, i+1, i+2) over n + 2 vertices; the ids ascending, descending or under a seeded permutation; -> (tris int32, V)"""
    V = n + 2
    i = np.arange(n, dtype=np.int64)
    t = np.stack([i, i + 1, i + 2], axis=1)
    rs = np.random.RandomState(seed)
    if order == "descending":
        t = V - 1 - t
    elif order == "permuted":
        t = rs.permutation(V)[t]
    elif order != "ascending":
        raise ValueError(order)
    if shuffle_triangles:
        t = t[rs.permutation(n)]
    return np.ascontiguousarray(t, dtype=np.int32), V


def fan(n):
    """n triangles (hub, 2i, 2i+1) with hub = V - 1: every hook contends on one word and the hub is never the root"""
    V = 2 * n + 1
    i = np.arange(n, dtype=np.int64)
    return np.ascontiguousarray(np.stack([np.full(n, V - 1), 2 * i, 2 * i + 1], axis=1), dtype=np.int32), V


def disjoint(n, seed=1):
    """n disjoint triangles under a permutation of the 3 n ids"""
    V = 3 * n
    return np.ascontiguousarray(np.random.RandomState(seed).permutation(V).reshape(n, 3), dtype=np.int32), V


def pad_inside(u, value):
    """a one-point frame of `value` around the volume (tests/test_oracle_geometry.py's, restated)"""
    p = np.full(tuple(s + 2 for s in u.shape), value, dtype=np.float32)
    p[1:-1, 1:-1, 1:-1] = u
    return p


def noise_volumes():
    """tests/test_gpu_geometry.py's own recipe, restated: -> (padded 33 x 29 x 31 uniform noise, open 17 x 40 x 23 noise with its transform)"""
    rs = np.random.RandomState(3)
    padded = pad_inside(rs.uniform(-1, 1, (31, 27, 29)).astype(np.float32), -1.0)
    opened = rs.uniform(-1, 1, (17, 40, 23)).astype(np.float32)
    return padded, (opened, dict(den=3.0, span=[1.0, 2.0, 3.0], lo=[0.5, -0.5, 0.0]))


FLOATER_SPHERES = (((0.0, 0.0, 0.0), 0.5), ((0.45, 0.0, 0.0), 0.2), ((0.8, 0.8, 0.8), 0.12), ((-0.8, 0.7, 0.0), 0.12), ((0.0, -0.85, 0.3), 0.04))


def body_with_floaters(n=40):
    """the maximum of the spheres r - |x - c| on linspace(-1, 1, n)^3: a body (two overlapping spheres) and three floaters"""
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return np.maximum.reduce([r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) for c, r in FLOATER_SPHERES]).astype(np.float32)


def mesh_checks(verts, tris):
    """closed + consistently oriented: every directed edge appears once and its reverse appears once (tests/test_oracle_geometry.py's, restated)"""
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * len(verts) + e[:, 1]
    rkey = e[:, 1] * len(verts) + e[:, 0]
    assert len(np.unique(key)) == len(key), "a directed edge is used twice: inconsistent orientation or a duplicated triangle"
    assert np.isin(rkey, key).all(), "an edge without its opposite: the surface has a hole"
    assert (tris[:, 0] != tris[:, 1]).all() and (tris[:, 1] != tris[:, 2]).all() and (tris[:, 0] != tris[:, 2]).all()
    assert len(np.unique(tris)) == len(verts), "every vertex is used"
