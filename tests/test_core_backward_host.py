"""CPU tier of the whole-backward tests (GPU tier: tests/test_gpu_core_backward.py): tests/golden/core_backward_bounds.json covers exactly the family-A
cases of tests/core_backward_cases.py and regenerates to the same bytes, no gradient case is degenerate, the drawn states hold the edges they claim and
the ray rule accepts N of 4 N candidates, family B's rule leaves enough rays on the golden view (estimated from the oracle's forward), and every bound
discriminates: mutants of the restatement miss it on the tensor they spoil."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import core_backward_cases as CC
from tests import field_op_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
CASES = CC.cases_a()


def generator():
    spec = importlib.util.spec_from_file_location("make_core_backward_bounds", os.path.join(ROOT, "tests", "golden", "make_core_backward_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rebuilt():
    G = generator()
    return G, G.build()


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(ROOT, "tests", "golden", "core_backward_bounds.json")) as f:
        return json.load(f)


def test_bounds_file_regenerates_to_the_same_bytes(rebuilt):
    G, doc = rebuilt
    with open(G.OUT) as f:
        assert f.read() == G.dumps(doc)


def test_bounds_file_covers_exactly_the_cases(bounds):
    assert bounds["rule"] == {"factor": CC.FACTOR, "floor": CC.FLOOR, "gmax_min": CC.GMAX_MIN, "legacy": CC.LEGACY} and CC.FACTOR == 4.0 and CC.FLOOR == 2.0 ** -21
    assert set(bounds["cases"]) == set(CASES) and 18 <= len(CASES) <= 22
    for cid, c in CASES.items():
        rec = bounds["cases"][cid]
        assert c["N"] * (c["T0"] + c["up"]) < 2000 and set(rec["tensors"]) == set(CC.TENSORS), cid
        assert all(len(v) == 3 and all(np.isfinite(q) and q >= 0.0 for q in v) for v in rec["tensors"].values()), cid
        assert rec["gmax"] >= CC.GMAX_MIN and rec["gmax"] == rec["tensors"]["g_W1"][2], cid
        # every tensor the case's upstreams reach has a gradient worth the name; the others are exactly zero in all three modes
        reached = {"g_" + k for k in FC.SDF_W} | set(FC.TABLE_TENSORS) | ({"g_" + k for k in FC.COLOR_W} if c["loss"] in ("all", "image") else set())
        if c["loss"] == "eikonal":                         # only the gradient carries an upstream: the +s and -s of an axis' two offset evaluations cancel in d b2
            reached.discard("g_b2")
            assert rec["tensors"]["g_b2"][2] < 1e-12, cid
        for k, (e32, eK, m64) in rec["tensors"].items():
            if k == "g_b2" and c["loss"] == "eikonal":
                continue
            if k in reached:
                assert m64 >= (1e-3 if k in FC.TABLE_TENSORS else CC.GMAX_MIN), (cid, k, m64)
            elif k != "g_inv_s":
                assert e32 == eK == m64 == 0.0, (cid, k)
        if c["loss"] == "eikonal":
            assert rec["tensors"]["g_inv_s"] == [0.0, 0.0, 0.0], cid
    n_open = 0
    for kind in ("widened", "open"):
        for name, e in bounds[kind].items():
            assert name in CC.TENSORS and e["cases"] and e["reason" if kind == "widened" else "note"], (kind, name)
            assert set(e["cases"]) <= set(CASES) | {"B/" + k for k in CC.CASES_B} | {"B/" + k + "/saved" for k in CC.CASES_B}, (kind, name)
            if kind == "widened":
                assert all(v["ratio"] > CC.FACTOR and v["ratio"] <= v["factor"] < 2.0 * max(v["ratio"], 4.0) + 1e-9 for v in e["cases"].values()), name
            else:
                n_open += len(e["cases"])
    assert n_open <= 3
    ids = set(CASES)
    assert {c["N"] for c in CASES.values()} == {1, 5, 37} and {(c["T0"], c["up"]) for c in CASES.values()} == {(16, 16), (32, 32), (40, 16), (2, 16)}
    assert {c["inv_s"] for c in CASES.values()} == {20.0, 300.0} and {c["car"] for c in CASES.values()} == {1.0, float(np.float32(0.3))}
    assert {c["weights"] for c in CASES.values()} == set(FC.WEIGHTS) and {c["loss"] for c in CASES.values()} == set(CC.UPSTREAMS)
    assert any(c["group_rays"] == 3 and c["N"] == 5 for c in CASES.values()) and sum(c["edges"] for c in CASES.values()) >= 4 and len(ids) == len(CASES)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_drawn_states_hold_what_they_claim(cid):
    """N of the 4 N candidate rays pass; every kept ray passes the three rules outside the samples placed on purpose, which are where they claim; no
    ReLU gate of the colour network and no side of |p| = 1.2 differs between float32 and float64"""
    c = CASES[cid]
    st = CC.draw_state(c)
    N, T = c["N"], c["T0"] + c["up"]
    assert c["N"] <= st["passed"] <= 4 * N and st["z"].shape == (N, T) and st["pts"].shape == (N, T, 3) and st["out16"].shape == (N, T, 16)
    pts, g, Wt = st["pts"].numpy(), st["gradient"].numpy(), FC.weights_of(c["weights"])
    ex_cos, ex_relax = np.zeros((N, T), bool), np.zeros((N, T), bool)
    assert set(st["where"]) == ({"inside", "outside", "zero_gradient", "clamped"} if c["edges"] else set())
    if c["edges"]:
        w = st["where"]
        ex_relax[w["inside"]] = ex_relax[w["outside"]] = ex_cos[w["zero_gradient"]] = True
        n_in, n_out = float(CC._norm32(pts[w["inside"]])), float(CC._norm32(pts[w["outside"]]))
        assert n_in < np.float32(1.2) <= n_out and 1.2 - n_in < 1e-6 and n_out - 1.2 < 1e-6
        assert (g[w["zero_gradient"]] == 0).all() and int((np.abs(g).sum(-1) == 0).sum()) == 1
        p = pts[w["clamped"]]
        assert 0 < FC.BOUND - p[2] < FC.EPS and FC.stencil_points(torch.from_numpy(p[None]).double())[5, 0, 2] == FC.BOUND
    else:
        assert (np.abs(g).sum(-1) > 0).all()
    gl = np.linalg.norm(g.astype(np.float64), axis=-1)
    assert gl[gl > 0].min() >= 0.1 - 1e-6 and gl.max() <= 2.0 + 1e-6
    assert CC.ray_rules(pts, g, st["out16"].numpy(), st["rays_d"].numpy(), Wt, ex_cos, ex_relax).all()
    assert FC.sdf_rows_pass(pts.reshape(-1, 3)).all()
    assert ((CC._norm32(pts) < np.float32(1.2)) == (np.linalg.norm(pts.astype(np.float64), axis=-1) < 1.2)).all()
    x, o = st["pts"].reshape(-1, 3), st["out16"].reshape(-1, 16)
    gates = None
    for dt in (torch.float32, F64):
        gg = st["gradient"].reshape(-1, 3).to(dt)
        h = torch.cat([x.to(dt), gg / (1e-5 + torch.linalg.norm(gg, dim=-1, keepdim=True)), o[:, 1:].to(dt)], -1)
        a1 = h @ Wt["Wc1"].to(dt).T
        a2 = a1.clamp(min=0) @ Wt["Wc2"].to(dt).T
        gates = gates or (a1 > 0, a2 > 0)
        assert torch.equal(gates[0], a1 > 0) and torch.equal(gates[1], a2 > 0)
    G = (N + c["group_rays"] - 1) // c["group_rays"] if c["group_rays"] else 1
    assert st["eik_den"].shape == (G,) and (st["up"]["eik"] is None or st["up"]["eik"].shape == (G,))
    assert {k for k, v in st["up"].items() if v is not None} == set(CC.UPSTREAMS[c["loss"]])


def test_the_straddling_tile_and_the_groups_are_there():
    """T = 56: ray 1 starts in the middle of a 16-row tile of the flat samples; two eikonal groups at N = 5 hold 3 and 2 rays with their own denominators"""
    assert any((c["T0"] + c["up"]) % 16 and c["N"] > 1 for c in CASES.values())
    st = CC.draw_state(CASES["n5-T16_16-s300-c1.0-golden-all-grp3"])
    relax = (np.linalg.norm(st["pts"].double().numpy(), axis=-1) < 1.2).sum(-1)
    assert np.allclose(st["eik_den"].numpy(), [relax[:3].sum() + 1e-5, relax[3:].sum() + 1e-5]) and st["eik_den"][0] != st["eik_den"][1]


# ---- family B ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def estimates():
    return {cid: CC.estimate_b(c) for cid, c in CC.CASES_B.items()}


def test_family_b_rule_leaves_enough_rays(estimates):
    """estimated from the oracle's forward (z_vals, sdf, gradient, color bit for bit the renderers'; out16 from the float32 restatement): at most a
    quarter of the rays zeroed -- the GPU tier fails above a half"""
    assert {k: (c["T0"], c["up"], c["rays"][0] * c["rays"][1], c["long"]) for k, c in CC.CASES_B.items()} == {
        "T16_16": (16, 16, 24, False), "T32_32": (32, 32, 12, False), "long-T40_16": (40, 16, 24, True)}
    for cid, (keep, st) in estimates.items():
        share = 1.0 - float(keep.mean())
        print(f"COREBWD B {cid} zeroed {share:.3f} of {len(keep)} rays")
        assert share <= CC.B_MAX_ESTIMATE, (cid, share)
        assert all(float(st["up"][k][~keep].abs().max() if (~keep).any() else 0.0) == 0.0 for k in ("image", "weights_sum", "depth", "normal_map"))


# ---- the bounds discriminate -------------------------------------------------------------------------------------------------------------------------------
def _miss(bounds, cid, names, mutant):
    """how many times its bound each named tensor of the mutant is off (float32 mutants of the restatement against the recorded bound)"""
    c = CASES[cid]
    m, r = CC.eval_a(c, (torch.float32, F64), mutant=mutant)[0], CC.eval_a(c, (F64,))[0]
    return [float(np.abs(m[k] - r[k]).max()) / CC.bound_of(*bounds["cases"][cid]["tensors"][k]) for k in names]


MUTANT_CASES = [("no_relax", "n37-T16_16-s300-c1.0-golden-eikonal", ("g_W1",)), ("k_with_c", "n37-T16_16-s300-c1.0-golden-normal_map", ("g_W1",)),
                ("no_comp_normal", "n37-T16_16-s300-c1.0-golden-normal_map", FC.TABLE_TENSORS), ("sdf_all_columns", "n37-T16_16-s300-c1.0-golden-all", ("g_W2",)),
                ("one_den", "n5-T16_16-s300-c1.0-golden-all-grp3", ("g_b1",)), ("recomputed_gradient", "n37-T16_16-s300-c1.0-golden-image", ("g_Wc1",))]


@pytest.mark.parametrize("mutant,cid,names", MUTANT_CASES, ids=[m[0] for m in MUTANT_CASES])
def test_the_bound_rejects_the_mutant(bounds, mutant, cid, names):
    miss = _miss(bounds, cid, names, mutant)
    print(f"COREBWD mutant {mutant} {cid} {min(miss):.3g} .. {max(miss):.3g} times the bound")
    assert min(miss) > 1.0, (mutant, cid, miss)


def test_the_unspoiled_restatement_stays_inside(bounds):
    """by construction of the rule -- on one thread, as the generator ran (a float32 sum depends on how torch splits it)"""
    cid = "n37-T16_16-s300-c1.0-golden-all"
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r32, rK, r64 = CC.eval_a(CASES[cid], (torch.float32, CC.K, F64))
    finally:
        torch.set_num_threads(threads)
    for m in (r32, rK):
        assert max(float(np.abs(m[k] - r64[k]).max()) / CC.bound_of(*bounds["cases"][cid]["tensors"][k]) for k in CC.TENSORS if r64[k].size) <= 0.25 + 1e-9


def test_family_b_bound_rejects_hi_times_hi_alone(estimates):
    """the saved-feature variant's dW1 with the lo parts dropped, against family B's own K bound (formed as the GPU tier forms it, on the estimated state)"""
    for cid in ("T16_16", "T32_32"):
        st = estimates[cid][1]
        r64, r32, rK = (CC.core_eval(st, m, own_cells=True) for m in (F64, torch.float32, CC.K_SAVED))
        mut = CC.core_eval(st, CC.K_SAVED, mutant="dw1_hi_only", own_cells=True)
        rows, ref, rec = CC.measure(r32, rK, r64, mut["rows"])
        err = float(np.abs(CC.on_rows(mut, rows)["g_W1"] - ref["g_W1"]).max())
        print(f"COREBWD mutant dw1_hi_only B/{cid} {err / CC.bound_of(*rec['g_W1']):.3g} times the bound")
        assert rec["g_W1"][2] >= CC.GMAX_MIN and err > CC.bound_of(*rec["g_W1"]), (cid, err, rec["g_W1"])
