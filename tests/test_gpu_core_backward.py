"""GPU tier of the whole-backward tests: nsr_ops.render_core_backward (ac_render_core_backward, csrc/render_core_backward.hip and the operators it
chains) called on a saved state and compared per tensor with float64 autograd of the chain at the saved values (tests/core_backward_cases.py).

Family A: every saved tensor drawn, feat7 = None (the re-gathering SDF backward); bounds from tests/golden/core_backward_bounds.json.
Family B: the state of a training forward on the golden field, read back; the backward once with feat7 (sdf_stencil_bwd_kernel<SAVED = true>) and once
without, bounds formed here from the three CPU modes on the state read back; rays the rule of CC.family_b_keep rejects are zeroed in every per-ray
upstream and stay in the launch.
Bound per tensor: 4 * max(err32, errK) + 2^-21 * max|f64|; a (case, tensor) under "widened" in the JSON takes its own factor, one under "open" the
tolerance the suite applied before (3e-4 of max|f64|); DESIGN.md section 5.2 has the reasons.  Exact expectations stay exact.  Every comparison prints
its figures (pytest -s) before it asserts: 'COREBWD family case tensor err err32 errK max64 bound'."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import core_backward_cases as CC
from tests import field_op_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _bounds():
    with open(os.path.join(ROOT, "tests", "golden", "core_backward_bounds.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def field(kind):
    """the Field of one weight set on the device, built once"""
    from avatarcraft_amd import nsr_ops
    p, Wt = FC.params(), FC.weights_of(kind)
    return nsr_ops.Field(torch.from_numpy(FC.table_of(kind)).to(DEV), p["offsets"], float(p["per_level_scale"]), FC.BASE,
                         *[Wt[k].to(DEV) for k in FC.SDF_W + FC.COLOR_W])


def dev(t):
    return None if t is None else t.detach().clone().contiguous().to(DEV)


def unpack(g_table, g_sdf_p, g_col_p, g_invs):
    """the operator's flat results -> {tensor: device tensor} and the whole-table gradient"""
    from avatarcraft_amd import nsr_ops
    names = ("g_W1", "g_b1", "g_W2", "g_b2", "g_Wc1", "g_Wc2", "g_Wc3")
    return dict(zip(names, nsr_ops.split_sdf_param_grads(g_sdf_p) + nsr_ops.split_color_param_grads(g_col_p)), g_inv_s=g_invs,
                g_table=g_table, flat=(g_sdf_p, g_col_p, g_invs))


def backward(f, opts, out, st, eik_groups=None):
    from avatarcraft_amd import nsr_ops
    up = {k: dev(v) for k, v in st["up"].items()}
    g_table = torch.zeros_like(f.t["table"])
    res = nsr_ops.render_core_backward(f, opts, out, dev(st["rays_o"]), dev(st["rays_d"]), dev(st["bg"]), up["image"], up["weights_sum"], up["depth"],
                                       up["normal_map"], up["eik"], g_table, eik_groups=eik_groups)
    torch.cuda.synchronize()
    return unpack(g_table, *res)


def same_bits(a, b, names=("g_table", "flat")):
    flat = lambda r: [t for k in names for t in (r[k] if isinstance(r[k], tuple) else (r[k],))]
    return all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(flat(a), flat(b)))


def touched_rows(got):
    return torch.nonzero(got["g_table"].abs().sum(1)).reshape(-1).cpu().numpy()


def on_rows(got, rows):
    """the operator's result as float64 arrays, the table gradient per level on the given rows of the whole table"""
    g = got["g_table"][torch.from_numpy(rows).to(DEV)].double().cpu().numpy()
    seg = np.searchsorted(rows, FC.table_offsets())
    res = {k: got[k].detach().double().cpu().numpy() for k in CC.WEIGHT_TENSORS + ("g_inv_s",)}
    res.update({name: g[seg[l]:seg[l + 1]] for l, name in enumerate(FC.TABLE_TENSORS)})
    return res


def check(fam, cid, got, ref64, rec):
    """every tensor against its bound; prints the figures first"""
    bad = []
    for name in CC.TENSORS:
        err32, errK, max64 = rec[name]
        wide = _bounds()["widened"].get(name, {}).get("cases", {}).get(cid if fam == "A" else "B/" + cid)
        bound = CC.bound_of(err32, errK, max64, wide["factor"] if wide else CC.FACTOR)
        if (cid if fam == "A" else "B/" + cid) in _bounds()["open"].get(name, {}).get("cases", {}):
            bound = CC.LEGACY * max64
        assert got[name].shape == ref64[name].shape, (fam, cid, name, got[name].shape, ref64[name].shape)
        err = float(np.abs(got[name] - ref64[name]).max()) if ref64[name].size else 0.0
        print(f"COREBWD {fam} {cid} {name} {err:.6e} {err32:.6e} {errK:.6e} {max64:.6e} {bound:.6e}")
        if not (np.isfinite(got[name]).all() and err <= bound):
            bad.append((name, err, err32, errK, max64, bound))
    assert not bad, (fam, cid, bad)


# ---- family A ----------------------------------------------------------------------------------------------------------------------------------------------
CASES = CC.cases_a()


def run_a(c, st):
    from avatarcraft_amd import nsr_ops
    f = field(c["weights"])
    N = c["N"]
    out = dict(z_vals=dev(st["z"]), pts=dev(st["pts"]), sdf=dev(st["sdf"]), sdf_out16=dev(st["out16"]), gradient=dev(st["gradient"]), color=dev(st["color"]))
    groups = None
    if c["group_rays"]:
        groups = (c["group_rays"], torch.stack([torch.zeros_like(st["eik_den"]), st["eik_den"]], -1).contiguous().to(DEV))
    else:
        out["eik_res"] = torch.cat([torch.zeros(1), st["eik_den"]]).to(DEV)
    opts = nsr_ops._render_opts(N, c["T0"], c["up"], FC.BOUND, False, float(st["inv_s"]), c["car"])
    return backward(f, opts, out, st, groups)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_drawn_state_matches_float64_autograd(cid):
    c = CASES[cid]
    st = CC.draw_state(c)
    st["geo"] = CC.geometry(st["pts"].reshape(-1, 3).numpy())
    got = run_a(c, st)
    r64 = CC.core_eval(st, F64)
    rows = CC.union_rows(r64["rows"], touched_rows(got))
    assert np.array_equal(rows, r64["rows"])               # every row the operator wrote to is a corner of the stencils (every other row is exactly zero)
    if c["loss"] not in ("all", "image"):                  # nothing reaches the colour: its network's weight gradients are exactly zero
        assert all(float(got[k].abs().max()) == 0.0 for k in ("g_Wc1", "g_Wc2", "g_Wc3"))
    check("A", cid, on_rows(got, rows), CC.on_rows(r64, rows), _bounds()["cases"][cid]["tensors"])
    assert same_bits(got, run_a(c, st))                    # a case repeats bit for bit


# ---- family B ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_b(cid):
    """the training forward of one family-B case -> (out, inputs, the state read back, the rays kept)"""
    from avatarcraft_amd import nsr_ops
    c = CC.CASES_B[cid]
    inp, f, inv_s = CC.inputs_b(c), field("golden"), float(FC.params()["inv_s"])
    t = lambda a: torch.from_numpy(a).to(DEV)
    render = nsr_ops.render_rays_long if c["long"] else nsr_ops.render_rays
    out = render(f, t(inp["rays_o"]), t(inp["rays_d"]), c["T0"], c["up"], FC.BOUND, inv_s, bg=t(inp["bg"]), noise=t(inp["noise"]), cos_anneal_ratio=CC.B_CAR,
                 extras=True, train_extras=True)
    torch.cuda.synchronize()
    assert ("feat7" in out) == (not c["long"])
    saved = {k: out[k].cpu().numpy() for k in ("z_vals", "pts", "sdf", "sdf_out16", "gradient", "color")}
    saved["eik_den"] = out["eik_res"][1:].cpu().numpy()
    keep = CC.family_b_keep(saved["pts"], saved["gradient"], saved["sdf_out16"], inp["rays_d"])
    print(f"COREBWD B {cid} zeroed {1.0 - keep.mean():.3f} of {len(keep)} rays")
    assert 1.0 - keep.mean() <= CC.B_MAX_ZEROED, (cid, keep)
    return out, inp, CC.state_b(c, inp, saved, inv_s, keep), keep


@functools.lru_cache(maxsize=None)
def modes_b(cid):
    """the CPU modes on the state read back, computed once: float64, float32 on its own cells, K and K with the saved-feature variant's dW1"""
    st = forward_b(cid)[2]
    return {m: CC.core_eval(st, m, own_cells=True) for m in (F64, torch.float32, CC.K) + (() if CC.CASES_B[cid]["long"] else (CC.K_SAVED,))}


def run_b(cid, saved_features):
    out, _, st, _ = forward_b(cid)
    if not saved_features:
        out = {k: v for k, v in out.items() if k != "feat7"}
    return backward(field("golden"), forward_b(cid)[0].opts, out, st)


def check_b(cid, got, mode_k, label):
    m = modes_b(cid)
    rows, ref, rec = CC.measure(m[torch.float32], m[mode_k], m[F64], touched_rows(got))
    assert rec["g_W1"][2] >= CC.GMAX_MIN and rec["g_Wc1"][2] >= CC.GMAX_MIN, rec
    check("B", label, on_rows(got, rows), ref, rec)


@pytest.mark.parametrize("cid", ["T16_16", "T32_32"])
def test_forward_state_matches_float64_autograd_with_and_without_saved_features(cid):
    saved, regather = run_b(cid, True), run_b(cid, False)
    check_b(cid, saved, CC.K_SAVED, cid + "/saved")
    check_b(cid, regather, CC.K, cid)
    # the compositor and the colour network do not know which SDF backward follows them
    assert same_bits(saved, regather, ("g_Wc1", "g_Wc2", "g_Wc3", "g_inv_s")) and torch.equal(saved["flat"][1], regather["flat"][1])
    assert same_bits(saved, run_b(cid, True)) and same_bits(regather, run_b(cid, False))
    _, _, st, keep = forward_b(cid)
    assert float(saved["g_inv_s"][torch.from_numpy(~keep).to(DEV)].abs().max() if (~keep).any() else 0.0) == 0.0      # a zeroed ray carries nothing


def test_forward_state_of_the_long_route():
    """the same rays through render_rays_long at 40 + 16 (T = 56, no feat7); where both routes apply the long forward equals the short one bit for bit"""
    from avatarcraft_amd import nsr_ops
    cid = "long-T40_16"
    got = run_b(cid, False)
    check_b(cid, got, CC.K, cid)
    assert same_bits(got, run_b(cid, False))
    c, f = CC.CASES_B["T16_16"], field("golden")
    assert np.array_equal(CC.rays_b(c)[0], CC.rays_b(CC.CASES_B[cid])[0]) and np.array_equal(CC.rays_b(c)[1], CC.rays_b(CC.CASES_B[cid])[1])
    short, inp = forward_b("T16_16")[0], forward_b("T16_16")[1]
    t = lambda a: torch.from_numpy(a).to(DEV)
    long = nsr_ops.render_rays_long(f, t(inp["rays_o"]), t(inp["rays_d"]), c["T0"], c["up"], FC.BOUND, float(FC.params()["inv_s"]), bg=t(inp["bg"]),
                                    noise=t(inp["noise"]), cos_anneal_ratio=CC.B_CAR, extras=True, train_extras=True)
    assert all(torch.equal(short[k], long[k]) for k in ("z_vals", "pts", "sdf", "sdf_out16", "gradient", "color", "image"))
