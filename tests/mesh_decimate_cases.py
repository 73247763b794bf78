"""The yardstick and the cases of the mesh-decimation tests (ac_mesh_cluster_count / _emit, csrc/mesh_cluster.hip; avatarcraft_amd/mesh_decimate.py): a plain numpy
restatement of the definitions of include/avatarcraft_hip.h -- the cell of a vertex by an fp64 subtraction, an fp64 division and np.floor, the clusters by
np.unique with first-occurrence ranks, the fixed-point sums by an int64 np.add.at, the position in the header's order of operations -- and the small meshes at which
the kernels can go wrong.  The reference has no counterpart.  Everything compared is an integer or a function of exact integer sums evaluated in one fixed order in
fp64: every comparison of these tests is exact equality, positions included.  CPU tier: tests/test_mesh_decimate_host.py; GPU tier: tests/test_gpu_mesh_decimate.py."""
import numpy as np

Q_ONE = float(2 ** 30)


def grid(lo, h, n):
    """a cluster grid as mesh_decimate.cluster_grid words it; a scalar lo or n is repeated on the three axes"""
    lo = [float(lo)] * 3 if np.ndim(lo) == 0 else [float(x) for x in lo]
    n = [int(n)] * 3 if np.ndim(n) == 0 else [int(x) for x in n]
    return dict(lo=lo, h=float(h), n=n)


def grid_over(lo, hi, h):
    """the grid of cell edge h from `lo` [3] that covers the box up to `hi` [3]"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return grid(lo, h, np.maximum(1, np.ceil((hi - lo) / h)).astype(np.int64))


def cells(vertices, g):
    """-> (valid [V] bool, cell [V,3] int64, q [V,3] int64, key [V] int64); rows of invalid vertices hold zeros"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    lo, h, n = np.asarray(g["lo"], np.float64), np.float64(g["h"]), np.asarray(g["n"], np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v - lo) / h
        valid = (np.isfinite(t) & (t >= 0) & (t < (n + 1).astype(np.float64))).all(axis=1)
    t = np.where(valid[:, None], t, 0.0)
    c = np.minimum(np.floor(t), (n - 1).astype(np.float64))
    f = t - c
    q = np.floor(f * Q_ONE).astype(np.int64)
    ci = c.astype(np.int64)
    key = (ci[:, 0] * n[1] + ci[:, 1]) * n[2] + ci[:, 2]
    return valid, ci, q, key


def cluster(vertices, triangles, g):
    """-> dict(cluster [V] int32, leader [V'] int32, members [V'] int32, positions [V',3] float64, triangles [T',3] int32, kept_triangles [T'] int32,
    bad_vertices, bad_triangles)"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    V = len(v)
    lo, h = np.asarray(g["lo"], np.float64), np.float64(g["h"])
    valid, ci, q, key = cells(v, g)
    idx = np.flatnonzero(valid)
    _, first, inv = np.unique(key[idx], return_index=True, return_inverse=True)      # first: the first (= smallest) valid vertex of every cell, in key order
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")                                           # cells by ascending leader
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    C = len(first)
    of_valid = rank[inv]
    cl = np.full(V, -1, np.int64)
    cl[idx] = of_valid
    leader = idx[first[order]]
    members = np.bincount(of_valid, minlength=C).astype(np.int64)
    S = np.zeros((C, 3), np.int64)
    np.add.at(S, of_valid, q[idx])
    cell = ci[leader].astype(np.float64)
    mean = S.astype(np.float64) / (members[:, None].astype(np.float64) * Q_ONE)
    positions = lo + (cell + mean) * h
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    in_range = ((t >= 0) & (t < V)).all(axis=1)
    ok = in_range.copy()
    ok[in_range] = valid[t[in_range]].all(axis=1)
    m = cl[t[ok]].reshape(-1, 3)
    alive = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    return dict(cluster=cl.astype(np.int32), leader=leader.astype(np.int32), members=members.astype(np.int32), positions=positions.reshape(-1, 3),
                triangles=m[alive].astype(np.int32).reshape(-1, 3), kept_triangles=np.flatnonzero(ok)[alive].astype(np.int32),
                bad_vertices=int((~valid).sum()), bad_triangles=int((~ok).sum()))


def edge_balance(triangles):
    """for every directed edge u -> v of the mesh, (its count) - (the count of v -> u): all zero for what is left of a closed oriented mesh after dropping
    collapsed triangles only (each collapsed triangle's two surviving edges are a pair u -> v, v -> u, and so are the edges that go with it)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(e.max()) + 1 if len(e) else 1
    fwd, fc = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    rev, rc = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
    return fwd, fc, rev, rc


def duplicate_triangles(triangles):
    """triangles that repeat an earlier one up to a rotation of its corners, or are the reverse of one (a back-to-back pair): -> (same orientation, opposite)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not len(t):
        return 0, 0
    r = np.argmin(t, axis=1)
    rot = np.stack([np.take_along_axis(t, ((r + k) % 3)[:, None], axis=1)[:, 0] for k in range(3)], axis=1)      # smallest corner first, orientation kept
    same = len(rot) - len(np.unique(rot, axis=0))
    flipped = rot[:, [0, 2, 1]]
    both = np.concatenate([np.unique(rot, axis=0), np.unique(flipped, axis=0)])
    opposite = (len(both) - len(np.unique(both, axis=0))) // 2
    return int(same), int(opposite)


# ---------------------------------------------------------------------------------------------------- cases
def strip_triangles(V):
    i = np.arange(max(V - 2, 0), dtype=np.int64)
    return np.ascontiguousarray(np.stack([i, i + 1, i + 2], axis=1), dtype=np.int32)


def random_mesh(V, T, n=4, seed=0):
    """V uniform vertices in a grid of n^3 unit cells from the origin (some on cell faces, one at the upper corner), T triangles: a strip and random ones.
    -> (vertices, triangles, grid)"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(0.0, n, (V, 3))
    v[::7] = np.floor(v[::7])                                                          # exactly on cell faces, edges and corners
    if V:
        v[V // 2] = n                                                                  # the upper corner: t = n, inside by the slack, clamped to the last cell
    t = np.concatenate([strip_triangles(V), rs.randint(0, max(V, 1), (T, 3)).astype(np.int32)])[:T] if V else np.zeros((0, 3), np.int32)
    return v, np.ascontiguousarray(t, dtype=np.int32), grid(0.0, 1.0, n)


def own_cells(V):
    """every vertex in a cell of its own: vertex i in the middle of cell (i % 50, (i // 50) % 50, i // 2500) of a 50^3 grid (V <= 125 000); a strip over them"""
    i = np.arange(V)
    v = np.stack([i % 50, (i // 50) % 50, i // 2500], axis=1) + 0.5
    return v.astype(np.float64), strip_triangles(V), grid(0.0, 1.0, 50)


def one_cell(V=70000, seed=4):
    """V vertices in ONE cell of a 3^3 grid (every add of the mesh lands on one slot; the sums reach V 2^29 ~ 2^45: not 32-bit), triangles among them"""
    rs = np.random.RandomState(seed)
    v = 1.0 + rs.uniform(0.0, 1.0, (V, 3))
    return v, strip_triangles(V), grid(0.0, 1.0, 3)


def far_cells(n_cells=4096, per_cell=3, seed=5):
    """n_cells occupied cells of a grid with 2^21 cells per axis, all in its upper half: keys from 2^62 / 2 up, far beyond 2^32 -- per_cell vertices each, the ids
    permuted; triangles at random (cells differ, most survive)"""
    rs = np.random.RandomState(seed)
    n = 2 ** 21
    c = rs.randint(n // 2, n, (n_cells, 3)).astype(np.float64)
    v = (np.repeat(c, per_cell, axis=0) + rs.uniform(0.0, 1.0, (n_cells * per_cell, 3)))[rs.permutation(n_cells * per_cell)]
    t = rs.randint(0, len(v), (2 * len(v), 3)).astype(np.int32)
    return np.ascontiguousarray(v), t, grid(0.0, 1.0, n)


def permuted(vertices, triangles, seed=6):
    """the same mesh with its vertex ids under a seeded permutation (new id of old vertex i = p[i]): the smallest id of a cell is no longer the first to arrive"""
    p = np.random.RandomState(seed).permutation(len(vertices))
    v = np.empty_like(vertices)
    v[p] = vertices
    return v, np.ascontiguousarray(p[np.asarray(triangles, np.int64)], dtype=np.int32)


def mc_grid(shape, k, den=1.0, span=(1.0, 1.0, 1.0), lo=(0.0, 0.0, 0.0)):
    """the cluster grid of k cells of the finest axis over a marching-cubes volume of `shape` whose vertices are index / den * span + lo"""
    step = np.asarray(span, np.float64) / den
    hi = np.asarray(lo, np.float64) + (np.asarray(shape, np.float64) - 1.0) * step
    return grid_over(lo, hi, float(k) * float(step.min()))
