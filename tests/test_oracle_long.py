"""CPU: the oracle's NeRFRenderer.run restatement over the long renderer's envelope (num_steps >= 2, upsample_steps a multiple of 16, at most 512
samples) against the reference's own run() at those counts (tests/golden/run_long.npz, tests/golden/make_long_golden.py).  The fixture's
searchsorted flips (`oracle_ss_flips`) are the oracle's: this file asserts that the oracle reproduces exactly them, so the GPU tier, which
holds the long renderer to the oracle bit for bit (tests/test_gpu_long_oracle.py), inherits the reference comparison."""
import numpy as np
import pytest

from tests.common import load_golden, make_rays, sort_orders_match_up_to_ties, LONG_INDEX_PASSES, LONG_INDEX_DIFFS

CASES = ["eval_128_128", "eval_100_64", "eval_256_0", "eval_96_32", "eval_40_16", "eval_16_496", "train_96_32"]


def _case(name):
    gd = load_golden("run_long.npz")
    pre = name + "/"
    return {k[len(pre):]: v for k, v in gd.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", CASES)
def test_long_counts_vs_reference(oracle, oracle_field, golden_params, name):
    c = _case(name)
    T0, up = int(c["num_steps"]), int(c["upsample_steps"])
    T, nup = T0 + up, up // 16
    r = oracle.render_rays(oracle_field, c["rays_o"], c["rays_d"], T0, up, 1.6, float(golden_params["inv_s"]), bg=c["bg"], noise=c.get("noise"))
    assert r["sort_index"].shape == (c["rays_o"].shape[0], max(nup, 1), max(T, 128))
    assert np.abs(r["image"] - c["image"]).max() <= 1e-3
    assert np.abs(r["weights_sum"] - c["weights_sum"]).max() <= 1e-3
    assert np.abs(r["depth"] - c["depth"]).max() <= 1e-3
    assert np.abs(r["normal_map"] - c["normal_map"]).max() <= 2e-3
    assert np.abs(r["z_vals"] - c["z_vals"]).max() <= 2e-3
    assert abs(r["gradient_error"] - float(c["gradient_error"])) <= 1e-4
    if not nup:
        assert np.array_equal(r["z_vals"], c["z_vals"])                                 # uniform samples: exact
        return
    # searchsorted indices: the reference's except at the recorded flips, each off by exactly 1
    npass = LONG_INDEX_PASSES.get(name, nup)
    flips = c["oracle_ss_flips"]
    assert (flips[:, 1] < npass).all()
    ss, ss_ref = r["ss_inds"], c["ss_inds"]
    bad = ss[:, :npass] != ss_ref[:, :npass]
    assert np.array_equal(np.argwhere(bad).astype(np.int32).reshape(-1, 3), flips), f"searchsorted flips {np.argwhere(bad).tolist()} != recorded {flips.tolist()}"
    assert (np.abs(ss[:, :npass].astype(np.int64) - ss_ref[:, :npass])[bad] == 1).all()
    assert int((ss != ss_ref).sum()) == LONG_INDEX_DIFFS.get(name, len(flips))      # the passes not compared (16 + 496): counted, not waved through
    sort_orders_match_up_to_ties(r["sort_index"][:, :npass, :T], c["sort_index"][:, :npass], flips)
    assert (r["sort_index"][:, :, T:] == -1).all()


@pytest.mark.parametrize("T0,up", [(400, 128), (512, 16), (1, 16), (0, 0), (64, 40), (17, 8)])
def test_out_of_envelope_counts_are_refused(oracle, oracle_field, T0, up):
    ro, rd = make_rays(2, 2, dist=1.7)
    with pytest.raises(RuntimeError, match="unsupported"):
        oracle.render_rays(oracle_field, ro, rd, T0, up, 1.6, 100.0)


def test_envelope_edges_render(oracle, oracle_field, golden_params):
    """the smallest and largest counts the envelope holds: T = 512 in one pass-free render and across 31 up-sampling passes (the sharpness
    64 * 2^30 of the last one is exact), and two coarse samples; every output finite and weights_sum in [0, 1]"""
    ro, rd = make_rays(4, 4, dist=1.7, f=4.0)
    for T0, up in ((512, 0), (2, 496), (2, 0), (17, 16)):
        r = oracle.render_rays(oracle_field, ro, rd, T0, up, 1.6, float(golden_params["inv_s"]))
        T = T0 + up
        assert r["z_vals"].shape == (16, T) and np.isfinite(r["image"]).all() and np.isfinite(r["z_vals"]).all()
        assert (np.diff(r["z_vals"], axis=1) >= 0).all(), (T0, up)                   # rays that hit the cube: sorted samples
        assert float(r["weights_sum"].min()) >= 0.0 and float(r["weights_sum"].max()) <= 1.0 + 1e-6


def test_near_far_rule(oracle, oracle_field, golden_params):
    """near_far = (near, far): a finite value replaces the cube's range (after its 0.05 clamp), +-inf keeps it -- the rule of the renderers'
    near_far argument (render_long.hip) and of the mesh-guided range (instant_nsr.py:148-153)"""
    ro, rd = make_rays(6, 6, dist=1.7, f=5.0)
    N, inv_s = ro.shape[0], float(golden_params["inv_s"])
    base = oracle.render_rays(oracle_field, ro, rd, 37, 32, 1.6, inv_s)
    inf = np.full(N, np.inf, np.float32)
    same = oracle.render_rays(oracle_field, ro, rd, 37, 32, 1.6, inv_s, near_far=(inf, -inf))
    for k in ("image", "z_vals", "weights", "sort_index", "ss_inds"):
        assert np.array_equal(same[k], base[k]), k
    near, far = oracle._near_far_cube(ro, rd, 1.6)
    nm, fm = (near + np.float32(0.3)).astype(np.float32), (far - np.float32(0.4)).astype(np.float32)
    nm[::3] = np.inf; fm[1::3] = -np.inf
    r = oracle.render_rays(oracle_field, ro, rd, 37, 0, 1.6, inv_s, near_far=(nm, fm))
    n_eff, f_eff = np.where(np.isinf(nm), near, nm), np.where(np.isinf(fm), far, fm)
    assert np.array_equal(r["z_vals"][:, 0], n_eff)                                  # lin_z[0] = 0: the first sample is near itself
    assert np.abs(r["z_vals"][:, -1] - f_eff).max() <= 1e-6 * np.abs(f_eff).max()   # near + span * 1
