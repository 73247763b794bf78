"""CPU: pin the oracle's occupancy-grid marcher away from the one grid, bound and camera of the A.4 known answers (tests/marcher_cases.py).

The second witness below is a scalar np.float32 restatement of the reference's two marching loops (kernel_march_rays_train and kernel_march_rays), written
from the algorithm: every arithmetic operation rounded once to fp32, the voxel index formed in double as the reference's `0.5 *` literal makes it, fmaxf /
fminf with their NaN rule (np.fmax / np.fmin), the generator a plain-integer pcg32.  It shares no code with oracle/ac_oracle_ops.c.  Step counts and
offsets must be equal, samples equal bit for bit."""
import numpy as np
import pytest

from tests import marcher_cases as MC

F = np.float32
_fmax, _fmin = np.fmax, np.fmin
_MASK64 = (1 << 64) - 1


class _Pcg32:
    """pcg32 (O'Neill, pcg-random.org minimal C implementation) with instant-ngp's next_float"""

    def __init__(self, initstate, initseq=1):
        self.state, self.inc = 0, ((initseq << 1) | 1) & _MASK64
        self.next_uint()
        self.state = (self.state + initstate) & _MASK64
        self.next_uint()

    def next_uint(self):
        old = self.state
        self.state = (old * 0x5851f42d4c957f2d + self.inc) & _MASK64
        xs, rot = (((old >> 18) ^ old) >> 27) & 0xffffffff, old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xffffffff

    def next_float(self):
        return np.array([(self.next_uint() >> 9) | 0x3f800000], np.uint32).view(np.float32)[0] - F(1)


def _clamp(x, lo, hi):
    return _fmin(hi, _fmax(lo, x))


class _Walk:
    """one ray of the reference's marcher: the shared set-up and the loop body"""

    def __init__(self, o, d, grid, mean_density, bound):
        self.o, self.d, self.grid = [F(v) for v in o], [F(v) for v in d], grid
        self.H, self.b = grid.shape[0], F(bound)
        self.rb = F(1) / self.b
        self.thresh = _fmin(F(10), F(mean_density))
        self.rd = [F(1) / v for v in self.d]
        self.dt_min = (F(2) * F(1.73205080757) / F(1024)) * self.b
        self.dt_max = F(2) * self.b / F(self.H - 1)
        self.dt_gamma = F(1) / F(256) if self.b > 1 else F(0)

    def near_far(self):
        ns, fs = [], []
        for a in range(3):
            n, f = (-self.b - self.o[a]) * self.rd[a], (self.b - self.o[a]) * self.rd[a]
            if n > f:
                n, f = f, n
            ns.append(n); fs.append(f)
        return _fmax(_fmax(ns[0], _fmax(ns[1], ns[2])), F(0.05)), _fmin(fs[0], _fmin(fs[1], fs[2]))

    def dt(self, t):
        return _clamp(t * self.dt_gamma, self.dt_min, self.dt_max)

    def march(self, t, far, max_samples):
        """-> list of (x, y, z, dt, t_after) for up to max_samples occupied positions in [t, far)"""
        H, b, hm1, out = self.H, self.b, F(self.H - 1), []
        while t < far and len(out) < max_samples:
            p = [_clamp(self.o[a] + t * self.d[a], -b, b) for a in range(3)]
            # the reference multiplies by a double 0.5: float -> double, two double products, back to float for the clamp, truncated
            v = [int(_clamp(F(0.5 * float(c * self.rb + F(1)) * float(H)), F(0), hm1)) for c in p]
            if self.grid[v[0], v[1], v[2]] > self.thresh:
                dt = self.dt(t)
                t = t + dt
                out.append((p[0], p[1], p[2], dt, t))
            else:
                tx = [(((F(v[a]) + F(0.5) + F(0.5) * np.copysign(F(1), self.d[a])) / hm1 * F(2) - F(1)) * b - p[a]) * self.rd[a] for a in range(3)]
                tt = t + _fmax(F(0), _fmin(tx[0], _fmin(tx[1], tx[2])))
                while True:
                    t = t + self.dt(t)
                    if not t < tt:
                        break
        return out


def witness_march_rays_train(rays_o, rays_d, grid, mean_density, bound, perturb, ray_ids):
    """kernel_march_rays_train for the rays `ray_ids` (their indices seed the jitter) -> per ray (near, t0, samples)"""
    res = []
    with np.errstate(all="ignore"):
        for n in ray_ids:
            w = _Walk(rays_o[n], rays_d[n], grid, mean_density, bound)
            near, far = w.near_far()
            t0 = near
            if perturb:
                t0 = t0 + w.dt_min * _Pcg32(int(n)).next_float()
            res.append((near, t0, w.march(t0, far, 1024)))
    return res


def witness_march_rays(n_step, rays_alive, rays_t, rays_o, rays_d, bound, grid, mean_density, far, perturb, slots):
    """kernel_march_rays for the alive slots `slots` -> per slot its samples (x, y, z, dt, t_after - last_t)"""
    res = []
    with np.errstate(all="ignore"):
        for n in slots:
            i = int(rays_alive[n])
            w = _Walk(rays_o[i], rays_d[i], grid, mean_density, bound)
            t = F(rays_t[n])
            if perturb:
                t = t + w.dt_min * _Pcg32(int(n), int(perturb)).next_float()
            last, rows = t, []
            for x, y, z, dt, ta in w.march(t, F(far[i]), n_step):
                rows.append((x, y, z, dt, ta - last)); last = ta
            res.append(rows)
    return res


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_ALL = MC.GRID_NAMES + ("kat129_r08",)


@pytest.fixture(scope="module")
def marched(oracle):
    """the oracle's training march of every case, computed once"""
    cache = {}

    def get(name, perturb):
        if (name, perturb) not in cache:
            g, mean, b = MC.grid(name)
            o, d = MC.rays(name)
            cache[name, perturb] = (o, d) + tuple(oracle.march_rays_train(o, d, g, mean, b, perturb=perturb))
        return cache[name, perturb]
    return get


def test_pcg32_witness_equals_the_oracles(oracle):
    for seed, seq in ((0, 1), (7, 1), (609, 1), (5, 3), (2 ** 40 + 3, 9)):
        a, b = _Pcg32(seed, seq), oracle.Pcg32(seed, seq)
        assert [a.next_uint() for _ in range(3)] == [b.next_uint() for _ in range(3)]
        assert float(a.next_float()) == b.next_float()


@pytest.mark.parametrize("name", sorted(MC.FIXED_STEP_COUNTS))
def test_known_step_counts_of_the_fixed_rays(marched, name):
    o, d, xyzs, dirs, deltas, rays, counter = marched(name, 0)
    assert rays[:MC.N_FIXED, 2].tolist() == MC.FIXED_STEP_COUNTS[name]
    assert np.array_equal(rays[:, 0], np.arange(len(o))) and np.array_equal(rays[1:, 1], np.cumsum(rays[:-1, 2]))
    m = int(counter[0])
    assert m == int(rays[:, 2].sum()) and np.isfinite(xyzs[:m]).all() and np.isfinite(deltas[:m]).all() and (deltas[:m] > 0).all()


def test_the_cases_reach_the_branches_they_are_there_for(marched):
    for name in MC.GRID_NAMES:
        o, d, xyzs, dirs, deltas, rays, counter = marched(name, 0)
        g, mean, b = MC.grid(name)
        assert len(o) == 610 and rays[MC.MISS_RAY, 2] == 0
        zero, neg = (d == 0) & ~np.signbit(d), (d == 0) & np.signbit(d)
        assert zero.any() and neg.any()
        if not name.startswith("corner"):
            assert (rays[zero.any(1), 2] > 0).any() and (rays[neg.any(1), 2] > 0).any()      # such rays take samples (and skips) too
            inside = np.abs(o).max(1) < b
            assert (rays[inside, 2] > 0).sum() >= 20                                          # origins inside the volume: the MIN_NEAR clamp
        near, far = MC.near_far(o, d, b)
        assert not np.isnan(near).any() and not np.isnan(far).any()
        assert (far < near).sum() >= 1 and far[MC.MISS_RAY] == -np.inf
    # bound <= 1: every step is dt_min; bound > 1: the proportional step t / 256 occurs (dt_max never wins at these distances)
    for name, kinds in (("unit33", {"min"}), ("half100", {"min"}), ("coarse17", {"gamma"}), ("noise37", {"gamma", "min"}), ("kat129", {"gamma", "min"})):
        o, d, xyzs, dirs, deltas, rays, counter = marched(name, 0)
        g, mean, b = MC.grid(name)
        dt_min, dt_max, _ = MC.step_sizes(b, g.shape[0])
        dl = deltas[:int(counter[0])]
        seen = {k for k, hit in (("min", (dl == dt_min).any()), ("max", (dl == dt_max).any()), ("gamma", ((dl > dt_min) & (dl < dt_max)).any())) if hit}
        assert kinds <= seen, (name, seen)
    # white noise: many alternations between samples and skips inside one batch of eight look-ups
    o, d, xyzs, dirs, deltas, rays, counter = marched("noise37", 0)
    g, mean, b = MC.grid("noise37")
    near, _ = MC.near_far(o, d, b)
    runs = [MC.sample_runs(o[n], d[n], b, 37, near[n], xyzs[rays[n, 1]:rays[n, 1] + rays[n, 2]]) for n in np.flatnonzero(rays[:, 2] >= 40)]
    assert max(runs) >= 20


@pytest.mark.parametrize("name", _ALL)
@pytest.mark.parametrize("perturb", [0, 1])
def test_training_march_equals_the_witness(marched, name, perturb):
    o, d, xyzs, dirs, deltas, rays, counter = marched(name, perturb)
    g, mean, b = MC.grid(name)
    ids = MC.witness_subset(len(o))
    assert len(ids) >= 30
    near_v, _ = MC.near_far(o, d, b)
    for n, (near, t0, smp) in zip(ids, witness_march_rays_train(o, d, g, mean, b, perturb, ids)):
        assert _bits(near) == _bits(near_v[n])
        assert rays[n, 2] == len(smp), (name, n, int(rays[n, 2]), len(smp))
        if not smp:
            continue
        off = int(rays[n, 1])
        assert off == int(rays[:n, 2].sum())
        w = np.array(smp, np.float32)
        sl = slice(off, off + len(smp))
        assert np.array_equal(_bits(xyzs[sl]), _bits(w[:, :3])), (name, n)
        assert np.array_equal(_bits(deltas[sl]), _bits(w[:, 3])), (name, n)
        assert np.array_equal(_bits(dirs[sl]), _bits(np.tile(d[n], (len(smp), 1)))), (name, n)


@pytest.mark.parametrize("name", MC.GRID_NAMES)
def test_inference_march_equals_the_witness(oracle, name):
    g, mean, b = MC.grid(name)
    o, d = MC.rays(name)
    N = len(o)
    near, far = MC.near_far(o, d, b)
    ids = MC.witness_subset(N)
    alive = ids[::-1].astype(np.int32).copy()
    # start positions: near, the middle of the span, just below far, above far
    with np.errstate(invalid="ignore"):
        kinds = [near[alive], (F(0.5) * (near[alive] + far[alive])).astype(np.float32), np.nextafter(far[alive], F(-np.inf)), (far[alive] + F(0.1)).astype(np.float32)]
    rt = np.choose(np.arange(len(alive)) % 4, kinds).astype(np.float32)
    rt[~np.isfinite(rt)] = F(0.05)
    for n_step, perturb in ((1, 0), (8, 0), (8, 3), (1024, 0)):
        xo, do_, dlo = oracle.march_rays(len(alive), n_step, alive, rt, o, d, b, g, mean, near, far, perturb)
        xo, do_, dlo = xo.reshape(-1, n_step, 3), do_.reshape(-1, n_step, 3), dlo.reshape(-1, n_step, 2)
        slots = np.arange(len(alive))
        for n, rows in zip(slots, witness_march_rays(n_step, alive, rt, o, d, b, g, mean, far, perturb, slots)):
            k = len(rows)
            assert (dlo[n, :, 0] != 0).sum() == k, (name, n_step, n)
            assert not xo[n, k:].any() and not dlo[n, k:].any()
            if k:
                w = np.array(rows, np.float32)
                assert np.array_equal(_bits(xo[n, :k]), _bits(w[:, :3])) and np.array_equal(_bits(dlo[n, :k]), _bits(w[:, 3:5])), (name, n_step, n)
                assert np.array_equal(_bits(do_[n, :k]), _bits(np.tile(d[alive[n]], (k, 1))))


@pytest.mark.parametrize("name", ["corner33", "corner64", "corner100"])
def test_diagonal_ray_reaches_recurrence_index_1024(oracle, name):
    """the input condition of the GPU tier's recorder-overflow test, from the oracle alone: the diagonal ray's last sample is position 1024 of its recurrence"""
    g, mean, b = MC.grid(name)
    o, d = MC.fixed_rays(b)
    o, d = np.stack([o[MC.DIAGONAL_RAY], -o[MC.DIAGONAL_RAY]]), np.stack([d[MC.DIAGONAL_RAY], -d[MC.DIAGONAL_RAY]])
    xyzs, dirs, deltas, rays, counter = oracle.march_rays_train(o, d, g, mean, b)
    near, _ = MC.near_far(o, d, b)
    k = MC.recurrence_indices(o[0], d[0], b, g.shape[0], near[0], xyzs[:rays[0, 2]])
    assert rays[0, 2] == {"corner33": 64, "corner64": 33, "corner100": 21}[name] and k.max() == 1024 and k.min() == 1025 - rays[0, 2]
    k1 = MC.recurrence_indices(o[1], d[1], b, g.shape[0], near[1], xyzs[rays[1, 1]:rays[1, 1] + rays[1, 2]])
    assert rays[1, 2] > 0 and k1.max() < 1024                  # reversed, the same voxels are the walk's first positions: recorded, not overflowed
    (_, _, smp), = witness_march_rays_train(o, d, g, mean, b, 0, [0])
    assert np.array_equal(_bits(np.array(smp, np.float32)[:, :3]), _bits(xyzs[:rays[0, 2]]))


def test_two_calls_accumulate_into_one_counter(oracle):
    g, mean, b = MC.grid("unit33")
    o, d = MC.rays("unit33")
    h = 301
    xa, da, la, ra, ca = oracle.march_rays_train(o[:h], d[:h], g, mean, b, perturb=1)
    xb, db, lb, rb, cb = oracle.march_rays_train(o[h:], d[h:], g, mean, b, perturb=1)
    ma, mb = int(ca[0]), int(cb[0])
    assert ma > 0 and mb > 0
    counter = np.zeros(2, np.int32)
    x1, d1, l1, r1, c1 = oracle.march_rays_train(o[:h], d[:h], g, mean, b, perturb=1, counter=counter)
    assert c1 is counter and counter.tolist() == [ma, h]
    x2, d2, l2, r2, c2 = oracle.march_rays_train(o[h:], d[h:], g, mean, b, perturb=1, counter=counter)
    assert counter.tolist() == [ma + mb, len(o)] and r2.shape == (len(o), 3) and x2.shape[0] >= ma + mb
    assert not r2[:h].any()                                          # the first call's rows belong to the first call's table
    shifted = rb.copy(); shifted[:, 1] += ma
    assert np.array_equal(np.concatenate([r1, r2[h:]]), np.concatenate([ra, shifted]))
    assert not x2[:ma].any() and not l2[:ma].any()                   # ... and so do its samples
    for got, first, second in ((x2, xa, xb), (d2, da, db), (l2, la, lb)):
        assert np.array_equal(_bits(got[ma:ma + mb]), _bits(second[:mb]))
    assert np.array_equal(_bits(x1[:ma]), _bits(xa[:ma])) and np.array_equal(_bits(l1[:ma]), _bits(la[:ma]))
    # a counter given as a plain sequence is copied, not written through
    out = oracle.march_rays_train(o[:5], d[:5], g, mean, b, counter=[37, 5])
    assert out[3].shape == (10, 3) and out[4].tolist() == [37 + sum(MC.FIXED_STEP_COUNTS["unit33"][:5]), 10] and out[3][5].tolist() == [0, 37, 263]
    with pytest.raises(ValueError):
        oracle.march_rays_train(o[:5], d[:5], g, mean, b, counter=[1, 2, 3])
