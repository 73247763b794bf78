"""CPU tier of the step-operator tests (GPU tier: tests/test_gpu_step_ops.py): tests/golden/step_op_bounds.json covers exactly the cases of
tests/step_op_cases.py, and the float64 restatements there reproduce what the reference itself recorded (tests/golden/run_train_64_64.npz,
nsr_params.npz) within the rule the GPU tier applies to the kernels: 4 * err32 + 2^-21 * max|f64| per tensor, err32 evaluated for that input."""
import json
import os

import numpy as np
import pytest
import torch

from tests import step_op_cases as SC
from tests.common import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(ROOT, "tests", "golden", "step_op_bounds.json")) as f:
        return json.load(f)


EXPECTED_TENSORS = {
    "composite": lambda c: set(SC.COMPOSITE_OUTPUTS) | (set(SC.COMPOSITE_GRADS) if c["grads"] else set()),
    "packed_shading": lambda c: set(SC.PACKED_OUTPUTS) | set(SC.PACKED_GRADS),
    "weight_norm": lambda c: {"w", "g_v", "g_g"},
    "variance": lambda c: {"g_variance"},
    "sds_upstream": lambda c: {"loss", "g_ws"},
}


def test_bounds_file_covers_exactly_the_cases(bounds):
    assert bounds["rule"] == {"factor": SC.FACTOR, "floor": SC.FLOOR, "gmax_min": SC.GMAX_MIN} and SC.FACTOR == 4.0 and SC.FLOOR == 2.0 ** -21
    fams = SC.families()
    assert set(bounds["families"]) == set(fams)
    for fam, (cases, _, is_grad) in fams.items():
        recs = bounds["families"][fam]
        assert set(recs) == set(cases), (fam, sorted(set(recs) ^ set(cases))[:5])
        for cid, c in cases.items():
            rec = recs[cid]
            assert set(rec["tensors"]) == EXPECTED_TENSORS[fam](c), (fam, cid)
            for k, (err32, max64) in rec["tensors"].items():
                assert np.isfinite(err32) and np.isfinite(max64) and err32 >= 0.0 and max64 >= 0.0, (fam, cid, k)
            assert ("gmax" in rec) == bool(is_grad(c)), (fam, cid)
            if is_grad(c):
                assert rec["gmax"] >= SC.GMAX_MIN and rec["gmax"] == max(rec["tensors"][k][1] for k in SC.GMAX_KEY[fam]), (fam, cid)
    for fam, w in bounds["widened"].items():
        for name, e in w.items():
            assert e["reason"] and e["cases"], (fam, name)
            for cid, m in e["cases"].items():
                assert cid.split("/")[0] in fams[fam][0] and name in EXPECTED_TENSORS[fam](fams[fam][0][cid.split("/")[0]]), (fam, name, cid)
                assert SC.FACTOR < m["ratio"] <= m["factor"] <= max(8.0, 2.0 * m["ratio"]), (fam, name, cid)


def test_bounds_file_is_not_stale(bounds):
    """a sample of every family, evaluated again in float64: the recorded max|f64| are those of today's generators"""
    for fam, (cases, evaluate, _) in SC.families().items():
        ids = sorted(cases, key=lambda cid: (cases[cid].get("N", 0) if isinstance(cases[cid], dict) else 0, cid))[:6]
        for cid in ids:
            r64 = evaluate(cases[cid], torch.float64)
            for k, (_, max64) in bounds["families"][fam][cid]["tensors"].items():
                now = float(np.abs(r64[k]).max()) if r64[k].size else 0.0
                assert abs(now - max64) <= 1e-9 * max64, (fam, cid, k, now, max64)


def test_composite_cases_hold_the_edges_they_claim():
    """alpha == 1 exactly in float32 on a large share of samples at inv_s >= 300, ray 1 starts inside the cube, ray 2 has both depth clamps active and
    weight on a clamped sample, and the many-ray launch starts with the 37-ray launch's rows"""
    cases = SC.composite_cases()
    c = cases["T32_64-s300-c1.0-bg-n37-all-b1.6"]
    inp = SC.composite_inputs(c)
    r32 = SC.composite_eval(c, inp, torch.float32)
    assert 0.2 <= float((r32["alpha"] == 1.0).mean()) <= 0.8
    assert float(inp["near"][1]) == float(np.float32(0.05))
    z, near, far = inp["z"].numpy(), inp["near"].numpy(), inp["far"].numpy()
    assert z[2, 0] < near[2] and z[2, -1] > far[2] and (np.diff(z, axis=-1) > 0).all()
    assert r32["weights"][2, 0] > 0.2                                        # (bg given: ray 2 meets the surface at its first sample, before near)
    small, big = SC.composite_inputs(cases["T16_16-s300-c1.0-bg-n37-all-b1.6"]), SC.composite_inputs(cases[f"T16_16-s300-c1.0-bg-n{SC.MANY_RAYS}-all-b1.6"])
    for k in ("rays_o", "rays_d", "z", "sdf", "normal", "color", "bg"):
        assert torch.equal(small[k], big[k][:37]), k
    for k in small["up"]:
        assert torch.equal(small["up"][k], big["up"][k][:37]), k


def test_a_wrong_last_delta_fails_d_sdf(bounds):
    """the cases whose ray 0 meets the surface at its last sample: the float32 restatement with the last delta taken as (far - near) / T instead of
    / num_steps misses the d sdf bound by orders of magnitude, whatever factor a case carries"""
    cases = {cid: c for cid, c in SC.composite_cases().items() if c["hit"] == "last"}
    assert len(cases) >= 10 and all(c["T0"] != c["T"] for c in cases.values())
    right = SC.composite_ref
    wrong = lambda z, sdf, normal, color, inv_s, rays_d, bg, near, far, num_steps, car: right(z, sdf, normal, color, inv_s, rays_d, bg, near, far, z.shape[1], car)
    for cid in sorted(cases)[::3]:
        c = cases[cid]
        inp = SC.composite_inputs(c)
        r64 = SC.composite_eval(c, inp, torch.float64)["g_sdf"]
        try:
            SC.composite_ref = wrong
            m32 = SC.composite_eval(c, inp, torch.float32)["g_sdf"]
        finally:
            SC.composite_ref = right
        err32, max64 = bounds["families"]["composite"][cid]["tensors"]["g_sdf"]
        assert float(np.abs(m32 - r64).max()) > 100.0 * (64.0 * err32 + SC.FLOOR * max64), cid


def _within(got, r32, r64, name):
    err32, max64 = float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
    err = float(np.abs(np.asarray(got, np.float64) - r64).max())
    assert err <= SC.bound_of(err32, max64), (name, err, err32, max64)


def test_compositing_half_reproduces_the_reference_recorded_render():
    """alpha, colour, z, bg and the rays the reference recorded for a 64 + 64 training render -> its weights, image, weights_sum and depth"""
    g = load_golden("run_train_64_64.npz")
    near, far = SC.cube_near_far(g["rays_o"], g["rays_d"], 1.6)
    res = {}
    for dt in (torch.float32, torch.float64):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        res[dt] = SC.to_np(SC.composite_from_alpha(t(g["alpha"]), t(g["color"]), t(g["z_vals"]), t(near), t(far), t(g["bg"])))
    for k in ("weights", "image", "weights_sum", "depth"):
        _within(g[k], res[torch.float32][k], res[torch.float64][k], k)


def test_weight_norm_ref_reproduces_the_stored_effective_matrices(golden_params):
    p = golden_params
    for W, layer in (("W1", "sdf_net.0"), ("W2", "sdf_net.1"), ("Wc1", "color_net.0"), ("Wc2", "color_net.1"), ("Wc3", "color_net.2")):
        v, g = torch.from_numpy(p[layer + ".weight_v"]), torch.from_numpy(p[layer + ".weight_g"])
        w32, w64 = SC.weight_norm_ref(v, g).numpy().astype(np.float64), SC.weight_norm_ref(v.double(), g.double()).numpy()
        _within(p[W], w32, w64, W)


def test_reference_gradients_at_the_edges_are_what_the_cases_say():
    """the float64 restatements at the exact edges: smooth-L1 of clamps passes the gradient at 0 and 1 and not outside; the variance clip gives 0"""
    c = SC.sds_cases()["pairs"]
    inp = SC.sds_inputs(c)
    r = SC.sds_eval(c, inp, torch.float64)
    ws, gt = inp["ws"].double().numpy(), inp["gt"].double().numpy()
    inside = (ws >= 0.0) & (ws <= 1.0)
    assert (r["g_ws"][~inside] == 0.0).all()
    expect = (np.clip(ws, 0, 1) - np.clip(gt, 0, 1)) * inp["scale"]
    assert np.array_equal(r["g_ws"][inside], expect[inside]) and (np.abs(expect[inside]) > 0).any()
    for v in SC.VARIANCE_CLIPPED:
        assert float(SC.variance_grad_ref(torch.tensor(v, dtype=torch.float64), torch.ones(5, dtype=torch.float64))) == 0.0
    c = SC.packed_cases()["M255-v248-d1-s300-c1.0"]
    r = SC.packed_eval(c, SC.packed_inputs(c), torch.float64)
    assert (r["eik"][248:] == 0.0).all() and (r["normal"][SC.packed_zero_rows(255)] == 0.0).all()
    assert np.abs(r["g_gradient_zero_rows"]).max() > 1e4                       # d normal / d g = I / 1e-5 on the rows with gradient == 0
