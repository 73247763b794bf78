"""The yardstick and the cases of the mesh-repair tests (ac_mesh_repair_count / _emit, csrc/mesh_repair.hip; avatarcraft_amd/mesh_repair.py): a plain numpy
restatement of the definition of include/avatarcraft_hip.h -- the uses of an edge by np.unique on (min, max) pairs, the order around a non-manifold edge by fp64
cross and dot products written out term by term in the header's order (never np.dot or np.cross: their order of operations is not the header's), the cyclic
bracket matching by a loop over a Python list, the fans by hooking and pointer jumping over the corner ids -- and the small meshes at which the kernels can go
wrong.  The reference has no counterpart.  Everything compared is an integer: every comparison of these tests is exact equality.  CPU tier: tests/test_mesh_repair_host.py;
GPU tier: tests/test_gpu_mesh_repair.py.  The marching-cubes fixtures are those of tests/mesh_component_cases.py, decimated and welded by the restatements of
tests/mesh_decimate_cases.py and tests/mesh_weld_cases.py."""
import numpy as np

from tests import mesh_decimate_cases as K
from tests import mesh_weld_cases as W

REPORT_KEYS = ("vertices", "split", "nonmanifold", "paired", "cut", "crowded", "invalid", "degenerate")
MAX_USES = 8


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def use_keys(P, a, b, opposite):
    """the keys of the uses of edge (a, b) whose opposite vertices are `opposite` (the first one is the use of smallest id) -> a list of np.float64"""
    with np.errstate(all="ignore"):
        pa = [np.float64(x) for x in P[a]]
        e = [np.float64(x) - y for x, y in zip(P[b], pa)]
        d = [[np.float64(x) - y for x, y in zip(P[c], pa)] for c in opposite]
        w = _cross(e, d[0])
        u = _cross(w, e)
        keys = []
        for di in d:
            X, Y = _dot(di, u), _dot(di, w)
            s = abs(X) + abs(Y)
            if s == 0:
                keys.append(np.float64(0.0))
                continue
            q = Y / s
            keys.append(q if (X >= 0 and Y >= 0) else (2.0 - q if X < 0 else 4.0 + q))
    return keys


def pair_uses(order, forward):
    """cyclic bracket matching over the use ids `order` (sorted around the edge): -> the list of joined (backward use, forward use)"""
    ring, pairs = list(order), []
    while True:
        for i, x in enumerate(ring):
            y = ring[(i + 1) % len(ring)]
            if not forward[x] and forward[y] and y != x:
                pairs.append((x, y))
                ring = [z for z in ring if z != x and z != y]
                break
        else:
            return pairs
        if not ring:
            return pairs


def fans(n, x, y):
    """the union-find over n corner ids by hooking and pointer jumping in numpy: x [m] and y [m] are united pairwise -> root [n], the smallest id of every set"""
    parent = np.arange(n, dtype=np.int64)
    while True:
        rx, ry = parent[x], parent[y]
        lo, hi = np.minimum(rx, ry), np.maximum(rx, ry)
        sel = lo != hi
        if not sel.any():
            return parent
        np.minimum.at(parent, hi[sel], lo[sel])                                           # a larger root goes under a smaller one
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up


def repair(vertices, triangles):
    """-> dict(triangles [T,3] int32, source [V'] int32, report: the eight counts and `added`)"""
    P = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    V = len(P)
    t, invalid, degenerate, member = W.classify(triangles, V)
    T = len(t)
    flat = t.reshape(-1)
    use = np.flatnonzero(np.repeat(member, 3))                                           # the use ids = the member corner ids, ascending
    k = use % 3
    nxt, opp = use - k + (k + 1) % 3, use - k + (k + 2) % 3                               # the corners at the end of the side and opposite
    p, q = flat[use], flat[nxt]
    lo, hi, fwd = np.minimum(p, q), np.maximum(p, q), p < q
    at_a, at_b = np.zeros(3 * T, np.int64), np.zeros(3 * T, np.int64)                     # use id -> its triangle's corner at a, at b
    at_a[use], at_b[use] = np.where(fwd, use, nxt), np.where(fwd, nxt, use)
    forward, opposite = np.zeros(3 * T, bool), np.zeros(3 * T, np.int64)                  # use id -> forward or not, its opposite corner
    forward[use], opposite[use] = fwd, opp
    joined = [np.zeros((0, 2), np.int64)]
    n_nonmanifold = n_paired = n_cut = n_crowded = 0
    if len(use):
        order = np.lexsort((use, hi, lo))
        lo_s, hi_s, use_s = lo[order], hi[order], use[order]
        start = np.flatnonzero(np.r_[True, (lo_s[1:] != lo_s[:-1]) | (hi_s[1:] != hi_s[:-1])])
        n_uses = np.diff(np.r_[start, len(use_s)])
        two = start[n_uses == 2]
        joined.append(np.stack([use_s[two], use_s[two + 1]], axis=1))                      # n = 2: joined, whatever their directions
        for s0, n in zip(start[n_uses > 2].tolist(), n_uses[n_uses > 2].tolist()):
            ids = use_s[s0:s0 + n].tolist()                                               # ascending: the first one is the reference use
            n_nonmanifold += 1
            keys = use_keys(P, int(lo_s[s0]), int(hi_s[s0]), flat[opposite[ids]].tolist()) if n <= MAX_USES else None
            if keys is None or not np.isfinite(keys).all():
                n_crowded += 1
                n_cut += n
                continue
            pairs = pair_uses([i for _, i in sorted(zip(keys, ids))], forward)
            joined.append(np.array(pairs, np.int64).reshape(-1, 2))
            n_paired += 2 * len(pairs)
            n_cut += n - 2 * len(pairs)
    j = np.concatenate(joined)
    parent = fans(3 * T, np.concatenate([at_a[j[:, 0]], at_b[j[:, 0]]]), np.concatenate([at_a[j[:, 1]], at_b[j[:, 1]]]))
    corners, vert = use, flat[use]
    root = parent[corners]
    first = np.full(V, 3 * T, np.int64)
    np.minimum.at(first, vert, root)
    extra = (root == corners) & (first[vert] != corners)
    extra_roots = corners[extra]                                                         # ascending
    rank = np.full(3 * T + 1, -1, np.int64)
    rank[extra_roots] = np.arange(len(extra_roots))
    out = flat.copy()
    out[corners] = np.where(first[vert] == root, vert, V + rank[root])
    source = np.concatenate([np.arange(V), vert[extra]])
    report = dict(vertices=V + len(extra_roots), split=len(np.unique(vert[extra])), nonmanifold=n_nonmanifold, paired=n_paired, cut=n_cut, crowded=n_crowded,
                  invalid=int(invalid.sum()), degenerate=int(degenerate.sum()))
    report["added"] = report["vertices"] - V
    return dict(triangles=out.astype(np.int32).reshape(-1, 3), source=source.astype(np.int32), report=report)


# ---------------------------------------------------------------------------------------------------- cases
TETRA_POINTS = [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5]]


def _outward(points, tris):
    """the triangles of a convex body, each flipped if need be so that its normal points away from the centroid"""
    P = np.asarray(points, np.float64)
    c = P[np.unique(tris)].mean(axis=0)
    out = []
    for a, b, d in tris:
        n = np.cross(P[b] - P[a], P[d] - P[a])
        out.append([a, b, d] if np.dot(n, P[a] - c) > 0 else [a, d, b])
    return out


def two_tetrahedra_on_an_edge():
    """two outward-oriented tetrahedra on either side of their common edge (0, 1) -> (vertices [6,3] float32, triangles [8,3] int32)"""
    P = TETRA_POINTS + [[-1.0, 0.0, 0.5], [0.0, -1.0, 0.5]]
    t = _outward(P, W.TETRAHEDRON) + _outward(P, np.array([0, 1, 4, 5])[np.array(W.TETRAHEDRON)].tolist())
    return np.array(P, np.float32), np.array(t, np.int32)


def two_tetrahedra_on_a_vertex():
    """two outward-oriented tetrahedra that share the vertex 0 only -> (vertices [7,3], triangles [8,3])"""
    P = TETRA_POINTS + [[-1.0, 0.0, -0.5], [0.0, -1.0, -0.5], [-1.0, -1.0, -1.0]]
    t = _outward(P, W.TETRAHEDRON) + _outward(P, np.array([0, 4, 5, 6])[np.array(W.TETRAHEDRON)].tolist())
    return np.array(P, np.float32), np.array(t, np.int32)


def fin():
    """a closed tetrahedron and a third triangle on its edge (0, 1) -> (vertices [5,3], triangles [5,3])"""
    P = TETRA_POINTS + [[-1.0, -1.0, 0.5]]
    return np.array(P, np.float32), np.array(_outward(P, W.TETRAHEDRON) + [[0, 1, 4]], np.int32)


def one_edge(n, seed=0, V=None):
    """n triangles that all use the edge (0, 1), in random directions and rotations, at random positions: their third corners all different (no other edge is
    used twice), or drawn from V - 2 vertices -> (vertices [V,3], triangles [n,3])"""
    rs = np.random.RandomState(seed)
    c = 2 + (rs.permutation(n) if V is None else rs.randint(0, V - 2, n))
    V = n + 2 if V is None else V
    P = rs.uniform(-1, 1, (V, 3)).astype(np.float32)
    t = np.where(rs.randint(0, 2, n)[:, None] == 0, np.stack([np.zeros(n, int), np.ones(n, int), c], 1), np.stack([np.ones(n, int), np.zeros(n, int), c], 1))
    r = rs.randint(0, 3, n)
    t = np.stack([np.take_along_axis(t, ((r + k) % 3)[:, None], axis=1)[:, 0] for k in range(3)], axis=1)
    return P, np.ascontiguousarray(t, dtype=np.int32)


def soup(V, T, seed=0, lattice=None):
    """T random triangles over V vertices at random positions, or on the integer lattice [0, lattice)^3: exact key ties, coplanar uses, coincident points"""
    rs = np.random.RandomState(seed)
    P = rs.uniform(-1, 1, (V, 3)) if lattice is None else rs.randint(0, lattice, (V, 3))
    return P.astype(np.float32), W.random_triangles(V, T, seed=seed + 1)


def random_positions(V, seed=0):
    return np.random.RandomState(seed).uniform(-1, 1, (V, 3)).astype(np.float32)


def welded(vertices, triangles, g):
    """marching-cubes mesh -> cluster -> weld by the restatements: -> (vertices [V,3] float32, triangles [T,3] int32)"""
    c = K.cluster(vertices, triangles, g)
    w = W.weld(c["triangles"], len(c["leader"]))
    return np.ascontiguousarray(c["positions"][w["kept_vertices"]], dtype=np.float32), w["triangles"]


def shell_volume(n=32):
    """the thin shell 0.04 - abs(r - 0.6) on linspace(-1, 1, n)^3"""
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (0.04 - np.abs(np.sqrt(x * x + y * y + z * z) - 0.6)).astype(np.float32)
