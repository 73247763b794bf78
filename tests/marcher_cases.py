"""Shared cases for the occupancy-grid marcher away from its one camera, grid and bound (tests/test_oracle_marcher_edges.py pins the oracle at them
with a second witness on the CPU, tests/test_gpu_marcher_edges.py pins the HIP operators to the oracle): grids of other sizes and bounds, and rays
with zero direction components (+0.0 and -0.0), origins inside the volume, on its boundary, on a voxel face, along the diagonal, and one that misses.
Everything is seeded numpy: both tiers rebuild the same arrays."""
import numpy as np

from tests.common import make_rays
from tests.test_oracle_kat import _sphere_grid as _sphere          # (H, bound, r): the grid of the A.4 known answers, so that kat129 stays that grid

F = np.float32


def _corner(H, lo):
    g = np.zeros((H, H, H), np.float32)
    g[lo:, lo:, lo:] = 100.0
    return g


def _noise(H, seed=37, fill=0.3):
    return (100.0 * (np.random.RandomState(seed).uniform(0, 1, (H, H, H)) < fill)).astype(np.float32)


# name -> (H, bound, builder, mean_density or None = the grid's own mean)
_GRIDS = {
    "unit33": (33, 1.0, lambda: _sphere(33, 1.0, 0.5), None),
    "half100": (100, 0.5, lambda: _sphere(100, 0.5, 0.25), None),
    "coarse17": (17, 2.0, lambda: _sphere(17, 2.0, 1.0), None),
    "noise37": (37, 1.6, lambda: _noise(37), None),
    "corner33": (33, 1.0, lambda: _corner(33, 30), 0.05),
    "kat129": (129, 1.6, lambda: _sphere(129, 1.6, 0.5), None),          # the grid of the existing known answers (control)
}
# the same corner block (the last three voxels of every axis) at bound 0.5, on a 64^3 grid and on half100's 100^3: the diagonal ray's last sample has
# recurrence index 1024 there too
_GRIDS["corner64"] = (64, 0.5, lambda: _corner(64, 61), 0.05)
_GRIDS["corner100"] = (100, 0.5, lambda: _corner(100, 97), 0.05)
# H = 129 at bound 1.6 with the sphere at half the bound, like the three small spheres: the grid the known step counts of the 129^3 row were taken on
# (kat129 keeps the radius 0.5 of the existing known answers)
_GRIDS["kat129_r08"] = (129, 1.6, lambda: _sphere(129, 1.6, 0.8), None)
GRID_NAMES = ("unit33", "half100", "coarse17", "noise37", "corner33", "kat129")
_CACHE = {}


def grid(name):
    """-> (density grid float32 [H,H,H] (read-only), mean_density, bound)"""
    if name not in _CACHE:
        H, bound, make, mean = _GRIDS[name]
        g = make()
        assert g.shape == (H, H, H)
        g.setflags(write=False)
        _CACHE[name] = (g, float(g.mean()) if mean is None else mean, bound)
    return _CACHE[name]


N_FIXED = 10
MISS_RAY = 4                     # index of the fixed ray that misses the volume
DIAGONAL_RAY = 5


def _normalised(d):
    d = np.asarray(d, np.float32)
    n = np.sqrt((d * d).sum(-1, keepdims=True, dtype=np.float32), dtype=np.float32)
    return (d / n).astype(np.float32)


def fixed_rays(b):
    """the ten hand-made rays, scaled by the bound b; directions normalised in fp32 (a zero component keeps its sign)"""
    o = np.array([[-3, .1, .2], [-3, .1, .2], [0, 0, 0], [0, 0, 0], [-3, 5, 0], [-2, -2, -2], [.1, 0, 3], [-3, 0, 0], [1, 0, 0], [0, -1, 0]], np.float64) * b
    d = np.array([[1, 0, 0], [1, -0.0, 0.0], [0, 0, 1], [.6, .64, .48], [1, 0, 0], [1, 1, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0]], np.float32)
    return o.astype(np.float32), _normalised(d)


def rays(name, n_inside=300, cam=(20, 15)):
    """-> rays_o, rays_d float32 [N,3] for the grid `name`: the fixed block, then n_inside seeded rays from origins inside the volume in random
    directions, then cam[0] x cam[1] camera rays scaled to the bound (N = 610 by default: three blocks of 256, the last one ragged)"""
    b = _GRIDS[name][1]
    fo, fd = fixed_rays(b)
    rs = np.random.RandomState(1000 + _GRIDS[name][0])
    io = rs.uniform(-b, b, (n_inside, 3)).astype(np.float32)
    idr = _normalised(rs.normal(0, 1, (n_inside, 3)).astype(np.float32))
    co, cd = make_rays(cam[0], cam[1], dist=1.8, f=0.75 * cam[1], yaw=0.6, pitch=-0.35)
    co = (co * F(b / 1.6)).astype(np.float32)
    return np.concatenate([fo, io, co]), np.concatenate([fd, idr, cd])


def witness_subset(n_rays, n_inside=300):
    """indices of the rays the scalar witness walks: the fixed block and a few dozen of the seeded rays of either family"""
    return np.concatenate([np.arange(N_FIXED), N_FIXED + np.arange(0, n_inside, 25), N_FIXED + n_inside + np.arange(0, n_rays - N_FIXED - n_inside, 25)])


# step counts of the ten fixed rays with perturb = 0 (the oracle's, pinned by the witness in tests/test_oracle_marcher_edges.py)
FIXED_STEP_COUNTS = {
    "unit33": [263, 268, 120, 120, 0, 268, 268, 263, 269, 264],
    "half100": [258, 260, 119, 119, 0, 283, 284, 294, 295, 294],
    "coarse17": [67, 70, 115, 129, 0, 69, 70, 67, 207, 196],
    "kat129_r08": [76, 76, 136, 138, 0, 74, 84, 84, 243, 242],
}


def near_far(o, d, bound):
    """the marcher's slab test (fp32, one rounding per operation, the reciprocal direction as the kernels form it) -> near, far [N]"""
    o, d, b = np.asarray(o, np.float32), np.asarray(d, np.float32), F(bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = F(1) / d
        n, f = (-b - o) * rd, (b - o) * rd
    sw = n > f
    n, f = np.where(sw, f, n), np.where(sw, n, f)
    near = np.fmax(np.fmax(n[:, 0], np.fmax(n[:, 1], n[:, 2])), F(0.05))
    far = np.fmin(f[:, 0], np.fmin(f[:, 1], f[:, 2]))
    return near.astype(np.float32), far.astype(np.float32)


def step_sizes(bound, H):
    """-> dt_min, dt_max, dt_gamma as fp32"""
    b = F(bound)
    return (F(2) * F(1.73205080757) / F(1024)) * b, F(2) * b / F(H - 1), (F(1) / F(256)) if bound > 1 else F(0)


def recurrence_indices(o, d, bound, H, t0, xyzs):
    """index in the ray's step recurrence t' = t + clamp(t dt_gamma, dt_min, dt_max) (from t0, fp32) of each of the ray's samples xyzs [n,3], found by
    replaying the recurrence on the host and matching the clamped positions bit for bit"""
    dt_min, dt_max, dt_gamma = step_sizes(bound, H)
    o, d, b = np.asarray(o, np.float32), np.asarray(d, np.float32), F(bound)
    xyzs = np.ascontiguousarray(xyzs, np.float32).reshape(-1, 3)
    ts, t = np.empty(1100, np.float32), F(t0)              # far - near <= the cube's diagonal = 1024 dt_min, and no step is shorter
    for k in range(len(ts)):
        ts[k] = t
        t = t + min(dt_max, max(dt_min, t * dt_gamma))
    pos = np.fmin(b, np.fmax(-b, o[None] + ts[:, None] * d[None])).astype(np.float32)
    out, k = [], 0
    for p in xyzs.view(np.uint32):
        hit = np.flatnonzero((pos[k:].view(np.uint32) == p).all(1))
        assert len(hit), "sample not on the recurrence"
        out.append(k + int(hit[0])); k = out[-1] + 1
    return np.array(out, np.int64)


def sample_runs(o, d, bound, H, t0, xyzs):
    """number of separate runs of consecutive recurrence positions among a ray's samples"""
    k = recurrence_indices(o, d, bound, H, t0, xyzs)
    return 0 if len(k) == 0 else 1 + int((np.diff(k) > 1).sum())
