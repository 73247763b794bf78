"""CPU tier of the field-operator tests (GPU tier: tests/test_gpu_field_ops.py): tests/golden/field_op_bounds.json covers exactly the cases of
tests/field_op_cases.py and is not stale, the inputs hold the edges they claim, the float64 restatements reproduce what the reference recorded
(tests/golden/field_points.npz), the table cubic of the declared-arithmetic mode is the kernels' own, and the bound discriminates: float32 mutants of
the restatement miss it."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import field_op_cases as FC
from tests.common import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(ROOT, "tests", "golden", "field_op_bounds.json")) as f:
        return json.load(f)


def test_bounds_file_covers_exactly_the_cases(bounds):
    assert bounds["rule"] == {"factor": FC.FACTOR, "floor": FC.FLOOR, "gmax_min": FC.GMAX_MIN} and FC.FACTOR == 4.0 and FC.FLOOR == 2.0 ** -21
    fams = FC.families()
    assert set(bounds["families"]) == set(fams)
    for fam, (cases, _, tensors) in fams.items():
        recs = bounds["families"][fam]
        assert set(recs) == set(cases), (fam, sorted(set(recs) ^ set(cases))[:5])
        for cid, c in cases.items():
            rec = recs[cid]
            assert set(rec["tensors"]) == set(tensors(c)), (fam, cid)
            for k, v in rec["tensors"].items():
                assert len(v) == 3 and all(np.isfinite(q) and q >= 0.0 for q in v), (fam, cid, k)
            assert rec["gmax"] >= FC.GMAX_MIN and rec["gmax"] == rec["tensors"][FC.GMAX_KEY[fam]][2], (fam, cid)
    for fam, w in bounds["open"].items():
        for name, e in w.items():
            assert fam in fams and e["cases"] and e["note"] and e["ratio"] > FC.FACTOR, (fam, name)
            assert all(cid in fams[fam][0] and name in fams[fam][2](fams[fam][0][cid]) for cid in e["cases"]), (fam, name)
    ids = set(FC.sdf_cases())
    assert {f"golden-all-nogx-b{B}" for B in (1, 15, 16, 17, 63, 65, 1000)} <= ids and {"drawn-all-nogx-b17", "drawn-all-nogx-b1000"} <= ids
    assert {"golden-sdf16-nogx-b65", "golden-normal-nogx-b65"} <= ids and {f"{w}-all-gx-b{B}" for w in FC.WEIGHTS for B in (1, 17, 1000)} <= ids
    ids = set(FC.color_cases())
    assert {f"golden-all-b{B}" for B in (1, 15, 16, 17, 63, 65, 1000)} | {"drawn-all-b17", "drawn-all-b1000", "golden-every_second_row_zero-b65"} == ids


def test_bounds_file_is_not_stale(bounds):
    """every case of up to 65 rows, evaluated again in float64: the recorded max|f64| are those of today's generators"""
    for fam, (cases, evaluate, _) in FC.families().items():
        for cid, c in cases.items():
            if c["B"] <= 65:
                r64, = evaluate(c, (F64,))
                for k, (_, _, max64) in bounds["families"][fam][cid]["tensors"].items():
                    now = float(np.abs(r64[k]).max()) if r64[k].size else 0.0
                    assert abs(now - max64) <= 1e-9 * max64, (fam, cid, k, now, max64)


def test_sdf_points_hold_what_they_claim():
    """every kept row passes both rejection rules; all 7 x 16 cells agree between float32 (fma and multiply-then-add) and float64; from 63 rows on the
    edge rows are there; the large launch starts with the small one's rows"""
    assert float(np.float32(FC.EPS)) == FC.EPS and float(np.float32(FC.BOUND)) == FC.BOUND
    for wk in FC.WEIGHTS:
        c = FC.sdf_case(1000, wk, gx=True)
        inp = FC.sdf_inputs(c)
        x = inp["x"].numpy()
        assert x.shape == (1000, 3) and FC.sdf_rows_pass(x).all() and np.abs(x).max() <= FC.BOUND
        pts = FC.stencil_points(inp["x"].double()).numpy()                   # (x +- eps rounds in float32: the margin covers 2048 * 2^-24 / 3.2 cells)
        p32 = FC.stencil_points(inp["x"]).numpy()
        cell = np.floor(FC.cell_positions(pts))
        assert np.array_equal(cell, np.floor(FC.cell_positions(p32, "f32_fma"))) and np.array_equal(cell, np.floor(FC.cell_positions(p32, "f32_mul_add")))
        assert np.array_equal(cell, FC.geometry(x)["cell"].numpy()) and cell.shape == (7, 1000, 16, 3)
        w = inp["where"]
        assert set(w) == set(FC.SDF_SPECIALS) and max(w.values()) < 63
        b, e = np.float32(FC.BOUND), FC.EPS
        assert x[w["on_plus_bound"], 0] == b and x[w["on_minus_bound"], 1] == -b and (x[w["corner"]] == [b, -b, b]).all()
        assert 0 < b - x[w["near_plus_bound"], 2] < e and 0 < x[w["near_minus_bound"], 0] + b < e
        assert pts[5, w["near_plus_bound"], 2] == FC.BOUND and pts[2, w["near_minus_bound"], 0] == -FC.BOUND        # the clamped offsets
        assert inp["where"] == FC.sdf_inputs(FC.sdf_case(63, wk, gx=True))["where"]
    small, big = FC.sdf_inputs(FC.sdf_case(FC.SMALL_LAUNCH, gx=True)), FC.sdf_inputs(FC.sdf_case(FC.large_launch(256), gx=True))
    assert len(big["x"]) == 16 * 12 * 256 + 5 and torch.equal(small["x"], big["x"][:37]) and all(torch.equal(small["up"][k], big["up"][k][:37]) for k in small["up"])
    assert FC.sdf_rows_pass(big["x"].numpy()).all()
    tail = FC.sdf_inputs(FC.sdf_case(FC.large_launch(256), gx=True), rows=slice(-5, None))
    assert torch.equal(tail["x"], big["x"][-5:]) and len(tail["up"]["out16"]) == 5


def test_drawn_weights_reach_the_knee_the_table_end_and_both_signs():
    """layer-1 pre-activations of the 7 points at 1000 rows: >= 5 % of (sample, unit) pairs in |100 a| < 4, in |a| >= 0.32 and in a > 0; every level of
    the drawn table is non-zero"""
    shares = {}
    for wk in FC.WEIGHTS:
        inp = FC.sdf_inputs(FC.sdf_case(1000, wk))
        geo, Wt = FC.geometry(inp["x"].numpy()), FC.weights_of(wk)
        pts = FC.stencil_points(inp["x"].double())
        feat, _ = FC.encode(pts, geo, torch.from_numpy(FC.table_of(wk)[geo["rows"]]).double())
        a = torch.cat([pts, feat], -1) @ Wt["W1"].double().T + Wt["b1"].double()
        shares[wk] = [float(m.double().mean()) for m in ((100.0 * a).abs() < 4.0, a.abs() >= 0.32, a > 0)]
        assert min(shares[wk]) >= 0.05, (wk, shares[wk])
    assert np.allclose(shares["golden"], [0.19, 0.17, 0.49], atol=0.02), shares["golden"]
    off, t = FC.table_offsets(), FC.table_of("drawn")
    assert t.dtype == np.float32 and all(np.abs(t[off[l]:off[l + 1]]).max() > 0 for l in range(16))


def test_color_inputs_hold_what_they_claim():
    for cid, c in FC.color_cases().items():
        if c["B"] < 63:
            continue
        inp, Wt = FC.color_inputs(c), FC.weights_of(c["weights"])
        x, n, o = (inp[k].double().numpy() for k in ("x", "normal", "out16"))
        assert FC.color_rows_pass(x, n, o, Wt).all(), cid
        assert np.linalg.norm(n, axis=-1).max() <= 1.0 + 1e-6 and inp["zero_row"] is not None and (n[inp["zero_row"]] == 0).all(), cid
        # no ReLU gate differs between the precisions
        h = torch.cat([inp["x"], inp["normal"], inp["out16"][:, 1:]], -1)
        for dt in (torch.float32, F64):
            a1 = h.to(dt) @ Wt["Wc1"].to(dt).T
            a2 = a1.clamp(min=0) @ Wt["Wc2"].to(dt).T
            gates = (a1 > 0, a2 > 0) if dt == torch.float32 else gates
            assert torch.equal(gates[0], a1 > 0) and torch.equal(gates[1], a2 > 0), cid
        if c["up"] == "every_second_row_zero":
            assert float(inp["up"][1::2].abs().max()) == 0.0 and float(inp["up"][0::2].abs().min()) > 0.0
    small, big = FC.color_inputs(FC.color_case(FC.SMALL_LAUNCH)), FC.color_inputs(FC.color_case(FC.large_launch(256)))
    assert all(torch.equal(small[k], big[k][:37]) for k in ("x", "normal", "out16", "up")) and len(big["x"]) == 16 * 12 * 256 + 5


def test_float64_restatement_reproduces_the_reference_recorded_points():
    """the 257 points of field_points.npz: sdf, gradient and colour within FACTOR * err32 + FLOOR * max|f64| evaluated for those inputs, the encoding
    within 1e-6 of the recorded float64 witness"""
    fp = load_golden("field_points.npz")
    x, geo, Wt, res = torch.from_numpy(fp["pts"]), FC.geometry(fp["pts"]), FC.weights_of("golden"), {}
    for dt in (torch.float32, F64):
        pts = FC.stencil_points(x.to(dt))
        feat, _ = FC.encode(pts, geo, torch.from_numpy(FC.table_of("golden")[geo["rows"]]).to(dt))
        out16, g = FC.sdf_query_ref(pts, feat, *[Wt[k].to(dt) for k in FC.SDF_W])
        n = g / (1e-5 + torch.linalg.norm(g, ord=2, dim=-1, keepdim=True))              # models/instant_nsr.py:215
        col = FC.color_ref(x.to(dt), n, out16, *[Wt[k].to(dt) for k in FC.COLOR_W])
        res[dt] = {k: v.double().numpy() for k, v in dict(sdf=out16, gradient=g, color=col, enc=feat[0]).items()}
    assert np.abs(res[F64]["enc"] - fp["enc_witness"]).max() < 1e-6
    for k in ("sdf", "gradient", "color"):
        r32, r64 = res[torch.float32][k], res[F64][k]
        err32, max64, err = float(np.abs(r32 - r64).max()), float(np.abs(r64).max()), float(np.abs(fp[k].astype(np.float64) - r64).max())
        assert err <= FC.FACTOR * err32 + FC.FLOOR * max64, (k, err, err32, max64)


def test_table_cubic_is_the_kernels_own():
    """tools/gen_softplus_table.fit(), which the declared-arithmetic mode evaluates, against the constants of csrc/ac_sp_table.hpp; and the table
    softplus against log1p(exp(100 x)) / 100 with its derivative against the sigmoid"""
    with open(os.path.join(ROOT, "avatarcraft_amd", "csrc", "ac_sp_table.hpp")) as f:
        vals = [float.fromhex(m) for m in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+", f.read())]
    tab = FC.softplus_table().numpy()
    assert tab.shape == (129, 4) and np.array_equal(np.asarray(vals, np.float32).reshape(129, 4), tab)
    x = torch.linspace(-0.4, 0.4, 200001, dtype=torch.float32).requires_grad_(True)
    y = FC.TableSoftplus.apply(x)
    y.sum().backward()
    x64 = x.detach().double()
    assert float((y.detach().double() - torch.nn.functional.softplus(x64, beta=100)).abs().max()) < 1e-7
    assert float((x.grad.double() - torch.sigmoid(100.0 * x64)).abs().max()) < 1e-4


def _miss(bounds, fam, cid, name, mutant, r64):
    """how many times its bound the mutant's tensor is off"""
    return float(np.abs(mutant[name] - r64[name]).max()) / FC.bound_of(*bounds["families"][fam][cid]["tensors"][name])


def test_the_bound_discriminates(bounds):
    """float32 mutants of the restatement, each against the bound of the tensor it spoils"""
    def sdf(cid, mode, mutant):
        c = FC.sdf_cases()[cid]
        inp = FC.sdf_inputs(c)
        geo = FC.geometry(inp["x"].numpy())
        return FC.sdf_eval(c, inp, mode, geo, mutant=mutant), FC.sdf_eval(c, inp, F64, geo)
    # the lo parts of W1^T d1 dropped: every level of the table gradient, with both weight sets
    for cid in ("golden-all-nogx-b1000", "drawn-all-nogx-b1000"):
        m, r = sdf(cid, FC.K, "drop_lo")
        miss = [_miss(bounds, "sdf_stencil", cid, k, m, r) for k in FC.TABLE_TENSORS]
        assert min(miss) > 2.0, (cid, miss)
    # the clamp passing its gradient: d x on the rows with a clamped offset
    m, r = sdf("golden-all-gx-b1000", torch.float32, "clamp_passes")
    assert _miss(bounds, "sdf_stencil", "golden-all-gx-b1000", "g_x", m, r) > 2.0
    # the clamp left out: the offset point leaves the cube and the encoder returns zeros there -- the table gradient of the rows with a clamped offset
    m, r = sdf("golden-all-gx-b1000", torch.float32, "no_clamp")
    miss = [_miss(bounds, "sdf_stencil", "golden-all-gx-b1000", k, m, r) for k in FC.TABLE_TENSORS]
    assert max(miss) > 2.0, miss
    # the difference divided by the clamped distance instead of eps
    m, r = sdf("golden-all-nogx-b1000", torch.float32, "div_clamped")
    assert _miss(bounds, "sdf_stencil", "golden-all-nogx-b1000", "gradient", m, r) > 2.0
    # the padding lanes of the last tile counted: the last row weighs 16 times at 17 rows
    m, r = sdf("golden-all-nogx-b17", torch.float32, "pad_lanes")
    assert _miss(bounds, "sdf_stencil", "golden-all-nogx-b17", "g_W1", m, r) > 2.0
    # the ReLU mask of layer 2 taken from layer 1
    c = FC.color_cases()["golden-all-b1000"]
    inp = FC.color_inputs(c)
    m, r = FC.color_eval(c, inp, torch.float32, mutant="relu2_from_l1"), FC.color_eval(c, inp, F64)
    assert _miss(bounds, "color_mlp", "golden-all-b1000", "g_Wc2", m, r) > 2.0
    # and the unspoiled float32 restatement and declared arithmetic stay inside, by construction of the rule
    for mode in (torch.float32, FC.K):
        ok = FC.color_eval(c, inp, mode)
        assert max(_miss(bounds, "color_mlp", "golden-all-b1000", k, ok, r) for k in FC.COLOR_TENSORS) <= 0.25 + 1e-9
