"""-m gpu: the occupancy-grid marcher (csrc/rm_device.hpp, raymarching.hip, the fused occupancy renderers of render_occupancy.hip) against the CPU oracle at
the cases of tests/marcher_cases.py -- grids of other sizes and bounds (bound <= 1: dt_gamma = 0; H = 17 .. 129, not powers of two), rays with +0.0 /
-0.0 direction components, origins inside the volume and on its boundary, a ray that misses, the diagonal ray whose last sample overflows the
recorder's 1024 positions, a non-zero counter on entry, both sides of the `>= M` cut, every exit of the inference compositor, and the single-workgroup
scan at and around its 1024 threads.  The oracle itself is pinned at these cases by a second witness (tests/test_oracle_marcher_edges.py).
Every comparison of the operators is exact: integers equal, floats bit for bit.  The fused renderers at the end are compared as the camera-ray tests of
tests/test_gpu_run_cuda.py compare them: bit for bit where those are, within their bounds elsewhere."""
import numpy as np
import pytest
import torch

from tests import marcher_cases as MC
from tests.gpu_common import assert_bitwise
from tests.test_gpu_run_cuda import env                      # noqa: F401  (the golden field + the oracle's 129^3 grid on the device, as a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)          # (a copy: the shared cases are read-only arrays)


@pytest.fixture(scope="module")
def marched(oracle):
    """the oracle's training march of a case, computed once and shared (read-only)"""
    cache = {}

    def get(name, perturb):
        if (name, perturb) not in cache:
            g, mean, b = MC.grid(name)
            o, d = MC.rays(name)
            res = (o, d) + tuple(oracle.march_rays_train(o, d, g, mean, b, perturb=perturb))
            for a in res:
                a.setflags(write=False)
            cache[name, perturb] = res
        return cache[name, perturb]
    return get


# ------------------------------------------------------------------ march_rays_train
@pytest.mark.parametrize("name", MC.GRID_NAMES)
@pytest.mark.parametrize("perturb", [0, 1])
def test_march_rays_train_equals_the_oracle(marched, name, perturb):
    import avatarcraft_amd.raymarching as RM
    o, d, xo, do_, dlo, ro, co = marched(name, perturb)
    g, mean, b = MC.grid(name)
    # what the case is there for, from the oracle's output alone
    assert len(o) == 610 and ro[MC.MISS_RAY, 2] == 0 and (ro[:, 2] == 0).sum() >= 1
    assert ((d == 0) & ~np.signbit(d)).any() and ((d == 0) & np.signbit(d)).any()
    if name == "noise37" and not perturb:
        near, _ = MC.near_far(o, d, b)
        assert max(MC.sample_runs(o[n], d[n], b, 37, near[n], xo[ro[n, 1]:ro[n, 1] + ro[n, 2]]) for n in np.flatnonzero(ro[:, 2] >= 40)) >= 20
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    x, dd, dl, rays = RM.march_rays_train(T(o), T(d), b, T(g), mean, 0, counter, -1, bool(perturb), -1, True)
    assert counter.cpu().tolist() == co.tolist()
    assert np.array_equal(rays.cpu().numpy(), ro)
    m = int(co[0])
    assert m > 0 and x.shape[0] == m
    assert_bitwise(x, xo[:m], "xyzs"); assert_bitwise(dd, do_[:m], "dirs"); assert_bitwise(dl, dlo[:m], "deltas")


@pytest.mark.parametrize("name", ["corner33", "corner64", "corner100"])
def test_recorder_overflow_walks_the_ray_again(oracle, name):
    """a sample at recurrence index >= 1024 does not fit the counting pass's record (RayRecorder: 32 words): the writer's second walk serves that ray.  The
    diagonal ray into the far corner block ends on index 1024; reversed, the block holds the walk's first positions and the record serves it."""
    import avatarcraft_amd.raymarching as RM
    g, mean, b = MC.grid(name)
    fo, fd = MC.fixed_rays(b)
    o = np.stack([fo[MC.DIAGONAL_RAY], -fo[MC.DIAGONAL_RAY], fo[0]])
    d = np.stack([fd[MC.DIAGONAL_RAY], -fd[MC.DIAGONAL_RAY], fd[0]])
    xo, do_, dlo, ro, co = oracle.march_rays_train(o, d, g, mean, b, perturb=0)
    near, _ = MC.near_far(o, d, b)
    k = [MC.recurrence_indices(o[n], d[n], b, g.shape[0], near[n], xo[ro[n, 1]:ro[n, 1] + ro[n, 2]]) for n in (0, 1)]
    assert k[0].max() >= 1024 and 0 < k[0].min() < 1024 and len(k[1]) > 0 and k[1].max() < 1024          # (a condition on the inputs, not on the kernel)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    x, dd, dl, rays = RM.march_rays_train(T(o), T(d), b, T(g), mean, 0, counter, -1, False, -1, True)
    assert counter.cpu().tolist() == co.tolist() and np.array_equal(rays.cpu().numpy(), ro)
    m = int(co[0])
    assert_bitwise(x, xo[:m], "xyzs"); assert_bitwise(dd, do_[:m], "dirs"); assert_bitwise(dl, dlo[:m], "deltas")


def test_a_counter_that_is_not_zero_on_entry(oracle):
    """the ABI accumulates (rays written from row counter[1], samples from counter[0]): two calls on the halves of a batch into one counter, through the
    backend with buffers sized for both (the Python wrapper sizes `rays` for one call from zero)"""
    from avatarcraft_amd.raymarching.backend import _backend
    g, mean, b = MC.grid("unit33")
    o, d = MC.rays("unit33")
    N, h, H = len(o), 301, g.shape[0]
    c_o = np.zeros(2, np.int32)
    oracle.march_rays_train(o[:h], d[:h], g, mean, b, perturb=1, counter=c_o)
    first = c_o.tolist()
    xo, do_, dlo, ro, _ = oracle.march_rays_train(o[h:], d[h:], g, mean, b, perturb=1, counter=c_o)
    xa, da, dla, ra, _ = oracle.march_rays_train(o[:h], d[:h], g, mean, b, perturb=1)
    total = int(c_o[0])
    assert first[0] > 0 and first[1] == h and total > first[0] and c_o[1] == N
    M = total + 64
    x, dd, dl = torch.zeros(M, 3, device=DEV), torch.zeros(M, 3, device=DEV), torch.zeros(M, device=DEV)
    rays = torch.zeros(N, 3, dtype=torch.int32, device=DEV)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    gt = T(g)
    _backend.march_rays_train(T(o[:h]), T(d[:h]), gt, mean, 0, b, h, H, M, x, dd, dl, rays, counter, 1)
    assert counter.cpu().tolist() == first
    _backend.march_rays_train(T(o[h:]), T(d[h:]), gt, mean, 0, b, N - h, H, M, x, dd, dl, rays, counter, 1)
    assert counter.cpu().tolist() == c_o.tolist()
    assert np.array_equal(rays.cpu().numpy(), np.concatenate([ra, ro[h:]]))
    m0 = first[0]
    for got, a, second, nm in ((x, xa, xo, "xyzs"), (dd, da, do_, "dirs"), (dl, dla, dlo, "deltas")):
        assert_bitwise(got[:m0], a[:m0], nm + " (first call)")
        assert_bitwise(got[m0:total], second[m0:total], nm + " (second call)")
        assert not bool(got[total:].any()), nm


@pytest.mark.parametrize("M", [263, 264, 300])
def test_the_sample_budget_cut(oracle, M):
    """`point_index + num_steps >= M` is a strict cut: the first fixed ray (263 samples from offset 0) is dropped at M = 263 and kept at 264; a cut ray keeps
    its row of the table, writes nothing, composites to zero and gets no gradient"""
    import avatarcraft_amd.raymarching as RM
    from avatarcraft_amd.raymarching.backend import _backend
    g, mean, b = MC.grid("unit33")
    o, d = MC.fixed_rays(b)
    N = len(o)
    xo, do_, dlo, ro, co = oracle.march_rays_train(o, d, g, mean, b, M=M)
    assert ro[:, 2].tolist() == MC.FIXED_STEP_COUNTS["unit33"]
    kept = (ro[:, 2] > 0) & (ro[:, 1] + ro[:, 2] < M)
    assert kept.tolist() == [M > 263] + [False] * 9                                   # both sides of the cut
    written = 263 if M > 263 else 0
    assert not xo[written:].any() and not dlo[written:].any() and (dlo[:written] > 0).all()
    x, dd, dl, rays = RM.march_rays_train(T(o), T(d), b, T(g), mean, 0, None, M, False, -1, False)
    assert x.shape == (M, 3) and dl.shape == (M,)
    assert np.array_equal(rays.cpu().numpy(), ro)
    assert_bitwise(x, xo, "xyzs"); assert_bitwise(dd, do_, "dirs"); assert_bitwise(dl, dlo, "deltas")       # the written prefix, and zeros behind it
    assert not bool(x[written:].any()) and not bool(dd[written:].any()) and not bool(dl[written:].any())
    # the packed compositor over that table
    rs = np.random.RandomState(M)
    sig = rs.uniform(0, 0.05, M).astype(np.float32); rgb = rs.uniform(0, 1, (M, 3)).astype(np.float32)
    ws_o, img_o = oracle.composite_rays_train_forward(sig, rgb, dlo, ro)
    assert not ws_o[~kept].any() and not img_o[~kept].any() and (ws_o[kept] > 0).all()
    sg, rg = T(sig).requires_grad_(True), T(rgb).requires_grad_(True)
    ws, img = RM.composite_rays_train(sg, rg, dl, rays, b)
    assert_bitwise(ws, ws_o, "weights_sum"); assert_bitwise(img, img_o, "image")
    gws = rs.normal(0, 1, N).astype(np.float32); gimg = rs.normal(0, 1, (N, 3)).astype(np.float32)
    (ws * T(gws)).sum().add((img * T(gimg)).sum()).backward()
    gs_o, gc_o = oracle.composite_rays_train_backward(gws, gimg, sig, rgb, dlo, ro, ws_o, img_o)
    assert_bitwise(sg.grad, gs_o, "grad_sigmas"); assert_bitwise(rg.grad, gc_o, "grad_rgbs")
    assert not gs_o[written:].any() and (gs_o[:written] != 0).any() == (written > 0)
    # the backward kernel leaves the rows of cut rays as it found them
    gs, gc = torch.full((M,), 7.0, device=DEV), torch.full((M, 3), 7.0, device=DEV)
    _backend.composite_rays_train_backward(T(gws), T(gimg), T(sig), T(rgb), dl, rays, ws.detach(), img.detach(), b, M, N, gs, gc)
    assert bool((gs[written:] == 7.0).all()) and bool((gc[written:] == 7.0).all())
    assert_bitwise(gs[:written], gs_o[:written], "grad_sigmas (prefix)"); assert_bitwise(gc[:written], gc_o[:written], "grad_rgbs (prefix)")


# ------------------------------------------------------------------ inference: march_rays, composite_rays, compact_rays
N_NEAR = 20          # the first rays are always alive and start at near: on the corner grids only rays 5 (the diagonal) and 13 meet the block


def _inference_inputs(name):
    g, mean, b = MC.grid(name)
    o, d = MC.rays(name)
    N = len(o)
    near, far = MC.near_far(o, d, b)
    rs = np.random.RandomState(N + g.shape[0])
    alive = np.concatenate([np.arange(N_NEAR), N_NEAR + rs.permutation(N - N_NEAR)[:601 - N_NEAR]]).astype(np.int32)        # 601 of the 610: ragged
    dt_min = MC.step_sizes(b, g.shape[0])[0]
    # start positions: near, the middle of the span, half a step and one ulp below far (the hardest against `t < far`), beyond far
    with np.errstate(invalid="ignore"):
        kinds = [near[alive], (np.float32(0.5) * (near[alive] + far[alive])).astype(np.float32), (far[alive] - np.float32(0.5) * dt_min).astype(np.float32),
                 np.nextafter(far[alive], np.float32(-np.inf)), (far[alive] + np.float32(0.1)).astype(np.float32)]
    rt = np.choose(np.arange(len(alive)) % 5, kinds).astype(np.float32)
    rt[:N_NEAR] = near[:N_NEAR]                                        # the first rays (the hand-made block among them) walk their whole span
    rt[~np.isfinite(rt)] = np.float32(0.05)                            # (the ray that misses: far = -inf)
    return g, mean, b, o, d, near, far, alive, rt


@pytest.mark.parametrize("name", MC.GRID_NAMES)
@pytest.mark.parametrize("n_step,perturb", [(1, 0), (8, 0), (8, 3), (1024, 0)])
def test_march_rays_equals_the_oracle(oracle, name, n_step, perturb):
    import avatarcraft_amd.raymarching as RM
    g, mean, b, o, d, near, far, alive, rt = _inference_inputs(name)
    n = len(alive)
    xo, do_, dlo = oracle.march_rays(n, n_step, alive, rt, o, d, b, g, mean, near, far, perturb)
    taken = (dlo.reshape(n, n_step, 2)[:, :, 0] != 0).sum(1)
    assert (taken == 0).any() and (taken > 0).any()
    if n_step <= 8:
        assert (taken == n_step).any()              # (at 1024 steps no walk can fill its slots: far - near <= 1024 dt_min and it starts behind near)
    x, dd, dl = RM.march_rays(n, n_step, T(alive), T(rt), T(o), T(d), b, T(g), mean, T(near), T(far), -1, perturb)
    assert_bitwise(x, xo, "xyzs"); assert_bitwise(dd, do_, "dirs"); assert_bitwise(dl, dlo, "deltas")


@pytest.mark.parametrize("name", MC.GRID_NAMES)
def test_composite_rays_on_those_deltas(oracle, name):
    import avatarcraft_amd.raymarching as RM
    g, mean, b, o, d, near, far, alive, rt = _inference_inputs(name)
    n, N, S = len(alive), len(o), 8
    _, _, dlo = oracle.march_rays(n, S, alive, rt, o, d, b, g, mean, near, far, 0)
    rs = np.random.RandomState(g.shape[0])
    sig = rs.uniform(0, 0.3, (n, S)).astype(np.float32)
    sig[2::3] = rs.uniform(0.9, 1.0, (len(sig[2::3]), S)).astype(np.float32)                # every third slot turns opaque within a few steps (on the corner
                                                                                            # grids slot 5 does and slot 13 does not: their two full rays)
    rgb = rs.uniform(0, 1, (n * S, 3)).astype(np.float32); nrm = rs.normal(0, 1, (n * S, 3)).astype(np.float32)
    acc = [rs.uniform(0, 0.3, N).astype(np.float32), rs.uniform(0, 2, N).astype(np.float32), rs.uniform(0, 1, (N, 3)).astype(np.float32),
           rs.normal(0, 1, (N, 3)).astype(np.float32)]                                        # the operator accumulates in place
    ref = [a.copy() for a in acc]
    rt_o = rt.copy()
    oracle.composite_rays(n, S, alive, rt_o, sig.reshape(-1), rgb, nrm, dlo, *ref)
    full = (dlo.reshape(n, S, 2)[:, :, 0] != 0).all(1)
    assert (rt_o[full] == -1).any()                                       # every step had a sample and the ray still stopped: T < 1e-2
    assert (rt_o >= 0).any()                                              # ran all its steps
    assert ((dlo.reshape(n, S, 2)[:, 0, 0] == 0) & (rt_o == -1)).any()    # no sample in the first slot: dl[0] == 0
    dev = [T(a) for a in acc]
    rt_g = T(rt)
    RM.composite_rays(n, S, T(alive), rt_g, T(sig.reshape(-1)), T(rgb), T(nrm), T(dlo), *dev)
    for a, r, nm in zip(dev + [rt_g], ref + [rt_o], ("weights_sum", "depth", "image", "normal_map", "rays_t")):
        assert_bitwise(a, r, nm)


@pytest.mark.parametrize("n_alive", [1, 63, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("pattern", ["all", "none", "mixed"])
def test_compact_rays_and_its_scan(oracle, n_alive, pattern):
    """the single-workgroup scan (1024 threads, ceil(n / 1024) elements each) below, at and above one element per thread, with empty and full results"""
    import avatarcraft_amd.raymarching as RM
    rs = np.random.RandomState(n_alive)
    ids = rs.permutation(5000)[:n_alive].astype(np.int32)
    t = rs.uniform(0.05, 3.0, n_alive).astype(np.float32)
    if pattern == "none":
        t[:] = -1
    elif pattern == "mixed":
        t[rs.uniform(0, 1, n_alive) < 0.4] = -1
        if n_alive > 1:
            t[0], t[-1] = -1, 0.0                      # t = 0 is alive (>= 0), the last element too
    ra_o, rt_o, cnt_o = oracle.compact_rays(n_alive, ids, t)
    assert cnt_o == {"all": n_alive, "none": 0}.get(pattern, cnt_o) and (pattern != "mixed" or n_alive == 1 or 0 < cnt_o < n_alive)
    ra = torch.full((n_alive,), -7, dtype=torch.int32, device=DEV); rt = torch.full((n_alive,), -7.0, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    RM.compact_rays(n_alive, ra, T(ids), rt, T(t), cnt)
    assert int(cnt[0]) == cnt_o
    assert np.array_equal(ra.cpu().numpy()[:cnt_o], ra_o[:cnt_o]); assert_bitwise(rt[:cnt_o], rt_o[:cnt_o], "rays_t")
    assert bool((ra[cnt_o:] == -7).all()) and bool((rt[cnt_o:] == -7.0).all())                 # nothing written behind the count


# ------------------------------------------------------------------ the fused occupancy renderers on the odd rays (golden field, bound 1.6)
def _odd_rays():
    return MC.rays("kat129", n_inside=150, cam=(15, 10))                 # 10 + 150 + 150 rays


def _oracle_single_round(O, of, o, d, grid, mean, inv_s, car):
    """the one launch's contract: the three operators run as a single round of 1024 steps from near_far_from_bound's near"""
    N = len(o)
    near, far = O._near_far_cube(o, d, 1.6)
    alive = np.arange(N, dtype=np.int32); rt = near.copy()
    xyzs, dirs, deltas = O.march_rays(N, 1024, alive, rt, o, d, 1.6, grid, mean, near, far)
    fs = O.field_samples(of, xyzs, dirs, deltas, 1.6, 0.005, inv_s, car)
    out = dict(weights_sum=np.zeros(N, np.float32), depth=np.zeros(N, np.float32), image=np.zeros((N, 3), np.float32), normal_map=np.zeros((N, 3), np.float32))
    O.composite_rays(N, 1024, alive, rt, fs["alpha"], fs["rgb"], fs["normal"], deltas, out["weights_sum"], out["depth"], out["image"], out["normal_map"])
    return out


@pytest.fixture(scope="module")
def grids(env):                                                          # noqa: F811
    """the oracle's 129^3 grid of the golden field, and a 65^3 one built the same way"""
    O = env["O"]
    g65, m65 = O.update_density_grid(env["of"], np.zeros((65,) * 3, np.float32), 1.6, resolution=65)
    return {129: (env["grid"], env["mean"]), 65: (g65, float(m65))}


@pytest.mark.parametrize("H", [129, 65])
def test_fused_inference_renderers_on_the_odd_rays(env, grids, H):       # noqa: F811
    from avatarcraft_amd import nsr_ops
    O, net = env["O"], env["net"].eval()
    o, d = _odd_rays()
    grid, mean = grids[H]
    car = 0.7
    ref = _oracle_single_round(O, env["of"], o, d, grid, mean, env["inv_s"], car)
    assert (ref["weights_sum"] == 0).any() and (ref["weights_sum"][:MC.N_FIXED] > 0.5).any() and (ref["weights_sum"][MC.N_FIXED:160] > 0.5).any()
    args = (net._field(), T(o), T(d), T(grid), mean, 1.6, 0.005, env["inv_s"], car)
    for phased in (False, True):
        out = nsr_ops.render_rays_occupancy(*args, phased=phased)
        for k in ("weights_sum", "depth", "image", "normal_map"):
            assert_bitwise(out[k], ref[k], f"{k} (phased={phased})")
    assert nsr_ops.occupancy_launch_failures() == 0
    # against the loop of rounds (oracle.run_cuda_eval): equal up to the one-ulp restarts of a round, the bounds of tests/test_gpu_run_cuda.py
    r = O.run_cuda_eval(env["of"], o, d, grid, mean, 1.6, 0.005, env["inv_s"], cos_anneal_ratio=car, bg=0.0)
    for k, kr in (("weights_sum", "weights_sum"), ("image", "image"), ("normal_map", "normal_map")):
        a = out[k].cpu().numpy()
        assert np.abs(a - r[kr]).max() <= 2e-5, k
        assert (a != r[kr]).mean() <= 0.01, k


@pytest.mark.parametrize("H", [129, 65])
@pytest.mark.parametrize("perturb", [0, 1])
def test_fused_training_renderer_on_the_odd_rays(env, grids, H, perturb):       # noqa: F811
    from avatarcraft_amd import nsr_ops
    import avatarcraft_amd.raymarching as RM
    O, net = env["O"], env["net"].eval()
    o, d = _odd_rays()
    N = len(o)
    grid, mean = grids[H]
    car = 0.7
    total = int(O.march_rays_train(o, d, grid, mean, 1.6, perturb=perturb)[4][0])
    assert total > 0
    for budget in (total, (2 * total) // 3):                             # a budget that fits, and one that leaves the later rays out
        r = O.run_cuda_train(env["of"], o, d, grid, mean, 1.6, 0.005, env["inv_s"], cos_anneal_ratio=car, bg=0.0, perturb=perturb, mean_count=budget)
        cap = budget + (128 - budget % 128)
        fits = (r["rays"][:, 2] > 0) & (r["rays"][:, 1] + r["rays"][:, 2] < cap)
        assert fits.any() and (budget == total or ((r["rays"][:, 2] > 0) & ~fits).any())
        # the chain of operators (run_cuda's train() branch under no_grad without the one launch) against the oracle: the bounds of
        # test_run_cuda_training_form_vs_oracle_chain
        field, ot, dt_, gt = net._field(), T(o), T(d), T(grid)
        c_chain = torch.zeros(2, dtype=torch.int32, device=DEV)
        xyzs, dirs, deltas, rays = RM.march_rays_train(ot, dt_, 1.6, gt, mean, 1, c_chain, budget, bool(perturb), 128, False)
        assert xyzs.shape[0] == cap and np.array_equal(rays.cpu().numpy(), r["rays"]) and c_chain.cpu().tolist() == r["counter"].tolist() == [total, N]
        ends = rays[:, 1] + rays[:, 2]
        n_valid = (ends * ((rays[:, 2] > 0) & (ends < cap))).max()
        valid = (torch.arange(cap, device=DEV) < n_valid).float()
        fs = nsr_ops.field_samples(field, xyzs, dirs, deltas, 1.6, 0.005, env["inv_s"], car, want_gradient=True)
        relax = (torch.linalg.norm(xyzs, ord=2, dim=-1) < 1.2).float() * valid
        gerr = (torch.linalg.norm(fs["gradient"], ord=2, dim=-1) - 1.0) ** 2
        g_chain = float((relax * gerr).sum() / (relax.sum() + 1e-5))
        ws_c, img_c = RM.composite_rays_train(fs["alpha"], fs["rgb"], deltas, rays, 1.6)
        _, nm_c = RM.composite_rays_train(fs["alpha"], fs["normal"].contiguous(), deltas, rays, 1.6)
        assert_bitwise(ws_c, r["weights_sum"], "weights_sum (chain)"); assert_bitwise(nm_c, r["normal_map"], "normal_map (chain)")
        assert np.abs(img_c.cpu().numpy() - r["image"]).max() <= 1e-6
        assert abs(g_chain - r["gradient_error"]) <= 1e-5 * max(1.0, r["gradient_error"])
        assert not r["weights_sum"][~fits].any()
        # the one launch against the chain: the bounds of test_training_form_in_one_launch_equals_the_chain_of_operators
        counter = torch.zeros(2, dtype=torch.int32, device=DEV)
        out = nsr_ops.render_rays_occupancy_train(field, ot, dt_, gt, mean, 1.6, 0.005, env["inv_s"], car, perturb=bool(perturb), capacity=cap,
                                                  composite_capacity=cap, counter=counter, bg=None)
        assert counter.cpu().tolist() == c_chain.cpu().tolist()
        assert_bitwise(out["weights_sum"], ws_c.cpu().numpy(), "weights_sum"); assert_bitwise(out["image"], img_c.cpu().numpy(), "image")
        assert_bitwise(out["normal_map"], nm_c.cpu().numpy(), "normal_map")
        g_one = float(out["gradient_error"])
        assert np.isfinite(g_one) and abs(g_chain - g_one) <= 2e-5 * max(1.0, abs(g_chain)), (g_chain, g_one)
