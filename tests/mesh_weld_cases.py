"""The yardstick and the cases of the mesh-weld tests (ac_mesh_weld_count / _emit, ac_mesh_topology, csrc/mesh_weld.hip; avatarcraft_amd/mesh_weld.py): a plain
numpy restatement of the definitions of include/avatarcraft_hip.h -- the groups by np.unique on sorted triples, the two leaders of a group by np.minimum.at, the
edges and their uses by np.unique on (min, max) pairs -- and the small index buffers at which the kernels can go wrong.  The reference has no counterpart.
Everything compared is an integer: every comparison of these tests is exact equality.  CPU tier: tests/test_mesh_weld_host.py; GPU tier:
tests/test_gpu_mesh_weld.py.  The marching-cubes fixtures are those of tests/mesh_component_cases.py and tests/mesh_decimate_cases.py."""
import numpy as np

REPORT_KEYS = ("vertices", "triangles", "invalid", "degenerate", "cancelled", "repeated", "excess")
TOPOLOGY_KEYS = ("edges", "boundary", "nonmanifold", "misoriented", "referenced", "faces", "invalid", "degenerate")


def classify(triangles, V):
    """-> (t [T,3] int64, invalid [T] bool, degenerate [T] bool, member [T] bool)"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    invalid = ~((t >= 0) & (t < V)).all(axis=1)
    degenerate = ~invalid & ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2]))
    return t, invalid, degenerate, ~invalid & ~degenerate


def signs(m):
    """the sign of every row of m [n,3] (three different corners): rotated so that the smallest corner comes first, (a, b, c), + iff b < c"""
    r = np.argmin(m, axis=1)
    b = np.take_along_axis(m, ((r + 1) % 3)[:, None], axis=1)[:, 0]
    c = np.take_along_axis(m, ((r + 2) % 3)[:, None], axis=1)[:, 0]
    return b < c


def weld(triangles, V):
    """-> dict(vertex_map [V], kept_vertices [V'], triangles [T',3], kept_triangles [T'], all int32; report: the seven counts)"""
    t, invalid, degenerate, member = classify(triangles, V)
    T = len(t)
    idx = np.flatnonzero(member)
    m = t[idx]
    plus = signs(m)
    if len(m):
        _, inv = np.unique(np.sort(m, axis=1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        G = int(inv.max()) + 1
    else:
        inv, G = np.zeros(0, np.int64), 0
    lead_plus, lead_minus = np.full(G, T, np.int64), np.full(G, T, np.int64)
    np.minimum.at(lead_plus, inv[plus], idx[plus])
    np.minimum.at(lead_minus, inv[~plus], idx[~plus])
    n_plus, n_minus = np.bincount(inv[plus], minlength=G), np.bincount(inv[~plus], minlength=G)
    net = n_plus - n_minus
    kept = np.sort(np.where(net > 0, lead_plus, lead_minus)[net != 0])
    assert (kept < T).all()
    used = np.zeros(V, bool)
    used[t[kept].reshape(-1)] = True
    vmap = np.full(V, -1, np.int64)
    vmap[used] = np.arange(int(used.sum()))
    report = dict(vertices=int(used.sum()), triangles=len(kept), invalid=int(invalid.sum()), degenerate=int(degenerate.sum()),
                  cancelled=int((n_plus + n_minus)[net == 0].sum()), repeated=int(((n_plus + n_minus)[net != 0] - 1).sum()),
                  excess=int((np.abs(net[net != 0]) - 1).sum()))
    assert T == report["triangles"] + report["invalid"] + report["degenerate"] + report["cancelled"] + report["repeated"]
    return dict(vertex_map=vmap.astype(np.int32), kept_vertices=np.flatnonzero(used).astype(np.int32), triangles=vmap[t[kept]].astype(np.int32).reshape(-1, 3),
                kept_triangles=kept.astype(np.int32), report=report)


def topology(triangles, V):
    """-> dict of ints: the eight counts, euler and closed_manifold"""
    t, invalid, degenerate, member = classify(triangles, V)
    m = t[member]
    e = np.concatenate([m[:, [0, 1]], m[:, [1, 2]], m[:, [2, 0]]])
    lo, hi, forward = e.min(axis=1), e.max(axis=1), e[:, 0] < e[:, 1]
    if len(e):
        _, inv = np.unique(np.stack([lo, hi], axis=1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        E = int(inv.max()) + 1
    else:
        inv, E = np.zeros(0, np.int64), 0
    fwd, bwd = np.bincount(inv[forward], minlength=E), np.bincount(inv[~forward], minlength=E)
    n = fwd + bwd
    r = dict(edges=E, boundary=int((n == 1).sum()), nonmanifold=int((n > 2).sum()), misoriented=int(((n == 2) & (fwd != bwd)).sum()),
             referenced=len(np.unique(m)), faces=len(m), invalid=int(invalid.sum()), degenerate=int(degenerate.sum()))
    r["euler"] = r["referenced"] - r["edges"] + r["faces"]
    r["closed_manifold"] = r["boundary"] == 0 and r["nonmanifold"] == 0 and r["misoriented"] == 0
    return r


def vertex_sets(triangles):
    """the sorted corner triples of the triangles, as a sorted list of tuples"""
    return sorted(map(tuple, np.sort(np.asarray(triangles, np.int64).reshape(-1, 3), axis=1).tolist()))


# ---------------------------------------------------------------------------------------------------- cases
TETRAHEDRON = [[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]]                              # closed, consistently oriented


def random_triangles(V, T, seed=0):
    """T triangles with corners uniform in [0, V): over a dozen vertices hundreds of members per group, both signs, many degenerate ones"""
    return np.ascontiguousarray(np.random.RandomState(seed).randint(0, V, (T, 3)), dtype=np.int32)


def sparse_triangles(V, T, seed=0):
    """T triangles over many vertices (V >> T: most vertices are orphans from the start), a third of them overwritten by a rotated or a reversed copy of
    another one, so that there are groups of both kinds all the same"""
    rs = np.random.RandomState(seed)
    t = rs.randint(0, V, (T, 3))
    dst, src = rs.permutation(T)[:T // 3], rs.randint(0, T, T // 3)
    copy = t[src]
    t[dst] = np.where((np.arange(len(dst)) % 2 == 0)[:, None], copy[:, [1, 2, 0]], copy[:, [2, 1, 0]])
    return np.ascontiguousarray(t, dtype=np.int32)


def one_set(n_plus, n_minus, corners=(3, 5, 7), seed=2):
    """n_plus + n_minus copies of ONE vertex set, each under a random rotation, the signs shuffled: every claim and every add of the mesh lands on one slot"""
    rs = np.random.RandomState(seed)
    a, b, c = sorted(corners)
    base = np.where(rs.permutation(n_plus + n_minus)[:, None] < n_plus, np.array([[a, b, c]]), np.array([[a, c, b]]))
    r = rs.randint(0, 3, len(base))
    t = np.stack([np.take_along_axis(base, ((r + k) % 3)[:, None], axis=1)[:, 0] for k in range(3)], axis=1)
    return np.ascontiguousarray(t, dtype=np.int32)


def high_indices(T=3000, pool=40, V=200_000, seed=3):
    """random triangles over `pool` vertex ids drawn from [2^16 + 1, V): groups with both signs whose sorted triples and edge keys do not fit 32 bits.
    -> (triangles, V)"""
    rs = np.random.RandomState(seed)
    ids = np.sort(rs.choice(np.arange(2 ** 16 + 1, V), pool, replace=False))
    return np.ascontiguousarray(ids[rs.randint(0, pool, (T, 3))], dtype=np.int32), V


def low_word_twins():
    """triangles (a, x, y) and (a + 2, x, y): their edges (a, x) and (a + 2, x) have keys (min << 31) | max that agree in the low 32 bits and differ above
    them, and the triangles differ in one corner only -- two closed tetrahedra that a 32-bit comparison would glue together.  -> (triangles, V)"""
    t = np.array(TETRAHEDRON, np.int64)
    a = np.array([2, 70_000, 70_001, 70_002])[t]
    b = np.array([4, 70_000, 70_001, 70_002])[t]
    return np.ascontiguousarray(np.concatenate([a, b]), dtype=np.int32), 70_003


def permuted_triangles(triangles, seed=6):
    """the same triangles in a seeded order: -> (triangles[p], p)"""
    p = np.random.RandomState(seed).permutation(len(triangles))
    return np.ascontiguousarray(np.asarray(triangles)[p]), p
