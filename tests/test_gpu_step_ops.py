"""GPU tier of the step-operator tests: the glue and compositing operators of a training step, called directly through their Python entries
(nsr_ops.composite, packed_shading, weight_norm_forward, weight_norm_all, param_grads, sds_upstream) and compared with float64 autograd of the
reference's own lines (tests/step_op_cases.py) at the shapes and edges the model never shows them.

Bound per tensor: 4 * err32 + 2^-21 * max|f64|, err32 = the float32-against-float64 error of the reference formulation itself, recorded by
tests/golden/make_step_op_bounds.py in tests/golden/step_op_bounds.json (no kernel involved); exact expectations stay exact.  A case whose gradient tensor
needs more than the factor 4 carries its own measured ratio and factor under "widened" there, with the reason per tensor.
Every comparison prints
its figures (pytest -s) before it asserts: 'STEPOP family case tensor err err32 max64 bound'."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import step_op_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _bounds():
    with open(os.path.join(ROOT, "tests", "golden", "step_op_bounds.json")) as f:
        return json.load(f)


def _np(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def _check_one(fam, cid, name, got, ref64, err32, max64):
    """-> None, or what is wrong with this tensor; prints the figures first"""
    wide = _bounds()["widened"].get(fam, {}).get(name, {}).get("cases", {}).get(cid)
    bound = (wide["factor"] if wide else SC.FACTOR) * err32 + SC.FLOOR * max64
    got = _np(got)
    assert got.shape == ref64.shape, (fam, cid, name, got.shape, ref64.shape)
    err = float(np.abs(got - ref64).max()) if ref64.size else 0.0
    print(f"STEPOP {fam} {cid} {name} {err:.6e} {err32:.6e} {max64:.6e} {bound:.6e}")
    return None if np.isfinite(got).all() and err <= bound else (fam, cid, name, err, err32, max64, bound)


def check(fam, cid, got, ref64, names=None):
    rec = _bounds()["families"][fam][cid]["tensors"]
    bad = [b for b in (_check_one(fam, cid, name, got[name], ref64[name], *rec[name]) for name in (names or sorted(rec))) if b]
    assert not bad, bad


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def dev(t, grad=False):
    return None if t is None else t.detach().clone().to(DEV).requires_grad_(grad)


# ---- composite -----------------------------------------------------------------------------------------------------------------------------------
COMPOSITE = SC.composite_cases()


def run_composite(c, inp, up=None):
    """-> {tensor: device tensor}: the six outputs and, for a gradient case, the four gradients of the case's loss (or of the given upstream weights)"""
    from avatarcraft_amd import nsr_ops
    sdf, nrm, col, inv_s = (dev(inp[k], c["grads"]) for k in ("sdf", "normal", "color", "inv_s"))
    out = nsr_ops.composite(dev(inp["z"]), sdf, nrm, col, inv_s, dev(inp["rays_o"]), dev(inp["rays_d"]), dev(inp["bg"]), c["T0"], c["bound"], c["car"])
    res = dict(zip(SC.COMPOSITE_OUTPUTS, out))
    if c["grads"]:
        SC.weighted_loss(res, {k: v.to(DEV) for k, v in (up or inp["up"]).items()}, SC.LOSSES[c["loss"]]).backward()
        res.update(g_sdf=sdf.grad, g_normal=nrm.grad, g_color=col.grad if col.grad is not None else torch.zeros_like(col), g_inv_s=inv_s.grad.reshape(-1))
    return {k: v.detach() for k, v in res.items()}


@pytest.mark.parametrize("cid", sorted(COMPOSITE))
def test_composite_matches_float64_autograd(cid):
    c = COMPOSITE[cid]
    inp = SC.composite_inputs(c)
    got = run_composite(c, inp)
    assert float(got["alpha"].min()) >= 0.0 and float(got["alpha"].max()) <= 1.0
    check("composite", cid, got, SC.composite_eval(c, inp, F64))
    again = run_composite(c, inp)
    assert same_bits([got[k] for k in sorted(got)], [again[k] for k in sorted(got)])                 # a case repeats bit for bit


@pytest.mark.parametrize("inv_s,car,bg", [(s, c, b) for s in SC.INV_S for c in SC.CARS for b in (True, False)])
def test_composite_ray_does_not_depend_on_the_launch(inv_s, car, bg):
    """the 37-ray launch against rows 0..36 of the launch of 4 * 4096 + 5 rays that starts with the same rays (the second trip of the grid-stride loop
    serves rays 16384..16388 from workgroups 0 and 1)"""
    small, big = SC._comp_case(16, 16, inv_s, car, bg, 37), SC._comp_case(16, 16, inv_s, car, bg, SC.MANY_RAYS)
    a, b = run_composite(small, SC.composite_inputs(small)), run_composite(big, SC.composite_inputs(big))
    keys = [k for k in sorted(a) if k != "g_inv_s"]                                                  # (summed over the launch's rays)
    assert same_bits([a[k] for k in keys], [b[k][:37] for k in keys])


@pytest.mark.parametrize("cid", ["T32_64-s300-c0.3-bg-n3-all-b1.6", "T36_100-s3000-c1.0-nobg-n3-all-b1.6", "T16_16-s20-c1.0-bg-n37-all-b1.6"])
def test_composite_inv_s_partial_per_ray(cid):
    """the operator returns the sum of the per-ray partials of d loss / d inv_s: with the upstream weights of all rays but one zeroed it is that ray's
    own value (the others add exact zeros), compared with the restatement's gradient for an inv_s leaf per ray under the same rule: err32 is the
    largest of the rays' float32 errors, max|f64| the largest partial"""
    c = COMPOSITE[cid]
    inp = SC.composite_inputs(c)
    r32, r64 = (SC.composite_eval(c, inp, dt, per_ray_inv_s=True)["g_inv_s"] for dt in (torch.float32, F64))
    assert r64.shape == (c["N"],)
    got = []
    for r in range(c["N"]):
        up = {k: torch.where((torch.arange(c["N"]) == r).reshape([-1] + [1] * (v.dim() - 1)), v, torch.zeros_like(v)) for k, v in inp["up"].items()}
        got.append(run_composite(c, inp, up)["g_inv_s"])
    assert not _check_one("composite", cid + "/per_ray", "g_inv_s", torch.cat(got), r64, float(np.abs(r32 - r64).max()), float(np.abs(r64).max()))


# ---- packed_shading ------------------------------------------------------------------------------------------------------------------------------
PACKED = SC.packed_cases()


def run_packed(c, inp):
    from avatarcraft_amd import nsr_ops
    sdf16, g, inv_s = (dev(inp[k], True) for k in ("sdf16", "gradient", "inv_s"))
    nv = torch.tensor([c["n_valid"]], dtype=torch.int32, device=DEV)
    out = nsr_ops.packed_shading(sdf16, g, inv_s, dev(inp["xyzs"]), dev(inp["dirs"]), dev(inp["deltas"]), nv, c["car"])
    res = dict(zip(SC.PACKED_OUTPUTS, out))
    SC.weighted_loss(res, {k: v.to(DEV) for k, v in inp["up"].items()}, SC.packed_loss_names(c)).backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    res.update(g_sdf16=zero(sdf16), g_gradient_all=g.grad, g_inv_s=zero(inv_s).reshape(-1))
    return {k: v.detach() for k, v in res.items()}


@pytest.mark.parametrize("cid", sorted(PACKED))
def test_packed_shading_matches_float64_autograd(cid):
    c = PACKED[cid]
    inp = SC.packed_inputs(c)
    got = run_packed(c, inp)
    ref = SC.packed_eval(c, inp, F64)
    assert float(got["alpha"].min()) >= 0.0 and float(got["alpha"].max()) <= 1.0
    eik = got["eik"].cpu().numpy()
    assert np.array_equal(eik[:, 1], ref["eik"][:, 1]) and (eik[c["n_valid"]:] == 0.0).all()         # relax is 0 or 1; padding rows have no eikonal share
    assert (eik[eik[:, 1] == 0.0, 0] == 0.0).all()
    assert float(got["g_sdf16"][:, 1:].abs().max()) == 0.0                                           # only column 0 is the sdf
    full = dict(got)
    full["g_gradient"], full["g_gradient_zero_rows"] = SC.packed_split(c, _np(got["g_gradient_all"]))
    check("packed_shading", cid, full, ref)
    again = run_packed(c, inp)
    assert same_bits([got[k] for k in sorted(got)], [again[k] for k in sorted(got)])


# ---- weight norm: forward ---------------------------------------------------------------------------------------------------------------------------
WN = SC.wn_cases()
SENTINEL = -77.0


def _wn_out(rows, cols, strided):
    """an output buffer filled with SENTINEL and the [rows, cols] view of it the kernel writes"""
    buf = torch.full((rows, cols + (SC.WN_PAD if strided else 0)), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[:, :cols]


def _wn_forward(ids, strided):
    from avatarcraft_amd import nsr_ops
    layers = [SC.wn_layer(*WN[i]) for i in ids]
    bufs = [_wn_out(*l["v"].shape, s) for l, s in zip(layers, strided)]
    nsr_ops.weight_norm_forward([(dev(l["v"]), dev(l["g"])) for l in layers], [w for _, w in bufs])
    torch.cuda.synchronize()
    for i, l, (buf, w), s in zip(ids, layers, bufs, strided):
        check("weight_norm", i, {"w": w}, SC.wn_eval(l, F64), names=["w"])
        if s:
            assert float((buf[:, w.shape[1]:] - SENTINEL).abs().max()) == 0.0, i                     # the padding of a row-strided destination stays


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("cid", [i for i in sorted(WN) if not i.startswith("full")])
def test_weight_norm_forward_one_layer(cid, strided):
    _wn_forward([cid], [strided])


def test_weight_norm_forward_full_launch_and_refusals():
    """AC_WN_MAX_LAYERS layers of mixed shapes in one launch (every second destination row-strided); one more, or an empty shape, is refused and
    nothing is launched"""
    from avatarcraft_amd import nsr_ops
    ids = [i for i in sorted(WN) if i.startswith("full")]
    assert len(ids) == SC.WN_MAX_LAYERS
    _wn_forward(ids, [k % 2 == 1 for k in range(len(ids))])
    layers = [SC.wn_layer(*WN[i]) for i in ids] + [SC.wn_layer(4, 5)]
    pairs = [(dev(l["v"]), dev(l["g"])) for l in layers]
    outs = [_wn_out(*l["v"].shape, False)[1] for l in layers]
    with pytest.raises(RuntimeError, match="weight_norm_forward"):
        nsr_ops.weight_norm_forward(pairs, outs)
    empty = (torch.empty((0, 5), dtype=torch.float32, device=DEV), torch.empty((0, 1), dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="weight_norm_forward"):
        nsr_ops.weight_norm_forward(pairs[:2] + [empty], outs[:2] + [torch.empty((0, 5), dtype=torch.float32, device=DEV)])
    torch.cuda.synchronize()
    assert all(float((w - SENTINEL).abs().max()) == 0.0 for w in outs)


# ---- weight norm: backward, bias and variance gradients (param_grads) -------------------------------------------------------------------------------
def _accumulated(fam, cid, name, got, old, g64, err32):
    """a destination after '+=': old + gradient, the gradient within its bound; the floor is four ulps of the largest SUM (the addition rounds once)"""
    want = old.double().numpy().reshape(g64.shape) + g64
    assert not _check_one(fam, cid, name, _np(got).reshape(g64.shape), want, err32, float(np.abs(want).max()))


class _Entries:
    """param_grads entries with the float64 expectation of every destination"""

    def __init__(self):
        self.entries, self.checks = [], []

    def weight_norm(self, cid, offset=0, pad=0):
        from avatarcraft_amd import nsr_ops
        l = SC.wn_layer(*WN[cid])
        rows, cols = l["v"].shape
        stride = cols + pad
        src = torch.full((offset + rows * stride,), 1e3, dtype=torch.float32)                        # (the gaps hold a value that would show in the sums)
        src[offset:].view(rows, stride)[:, :cols] = l["gw"]
        dv, dg = dev(l["old_v"]).clone(), dev(l["old_g"]).reshape(-1).clone()
        self.entries.append((nsr_ops.PG_WEIGHT_NORM, (src.to(DEV), offset) if offset else src.to(DEV), stride, rows, cols, dev(l["v"]), dev(l["g"]), dv, dg))
        ref, rec = SC.wn_eval(l, F64), _bounds()["families"]["weight_norm"][cid]["tensors"]
        self.checks += [("weight_norm", cid, "g_v", dv, l["old_v"], ref["g_v"], rec["g_v"][0]), ("weight_norm", cid, "g_g", dg, l["old_g"], ref["g_g"], rec["g_g"][0])]

    def add(self, rows, stride):
        from avatarcraft_amd import nsr_ops
        a = SC.add_inputs(rows, stride)
        dst = dev(a["old"]).clone()
        self.entries.append((nsr_ops.PG_ADD, dev(a["src"]).reshape(-1), stride, rows, 0, None, None, dst, None))
        self.checks.append(("add", f"r{rows}s{stride}", "dst", dst, a["old"], a["src"][:, 0].double().numpy(), 0.0))

    def variance(self, cid):
        from avatarcraft_amd import nsr_ops
        c = SC.variance_cases()[cid]
        a = SC.variance_inputs(c)
        inv_s = nsr_ops.variance_forward(dev(a["variance"]))
        dst = dev(a["old"]).clone()
        self.entries.append((nsr_ops.PG_VARIANCE, dev(a["rows"]), 1, c["rows"], 0, None, inv_s.reshape(-1), dst, None))
        ref = SC.variance_eval(c, a, F64)["g_variance"]
        self.checks.append(("variance", cid, "g_variance", dst, a["old"], ref, _bounds()["families"]["variance"][cid]["tensors"]["g_variance"][0]))
        if c["variance"] in SC.VARIANCE_CLIPPED:
            assert float(ref[0]) == 0.0 and float(inv_s) in (float(np.float32(1e-6)), float(np.float32(1e6)))
            self.exact = getattr(self, "exact", []) + [(dst, a["old"])]

    def launch_and_check(self, order=None):
        from avatarcraft_amd import nsr_ops
        order = list(range(len(self.entries))) if order is None else order
        nsr_ops.param_grads([self.entries[i] for i in order], torch.device(DEV))
        torch.cuda.synchronize()
        for ch in self.checks:
            _accumulated(*ch)
        for dst, old in getattr(self, "exact", []):
            assert torch.equal(dst.cpu(), old)                                                       # outside the clip range exactly nothing is added


@pytest.mark.parametrize("cid", [i for i in sorted(WN) if not i.startswith("full")])
@pytest.mark.parametrize("offset,pad", [(0, 0), (5, 4)])
def test_param_grads_weight_norm(cid, offset, pad):
    """one layer's backward into destinations that already hold values; src given as (tensor, element offset) with src_stride > cols"""
    e = _Entries()
    e.weight_norm(cid, offset, pad)
    e.launch_and_check()


@pytest.mark.parametrize("rows,stride", SC.ADD_CASES)
def test_param_grads_add(rows, stride):
    e = _Entries()
    e.add(rows, stride)
    e.launch_and_check()


@pytest.mark.parametrize("cid", sorted(SC.variance_cases()))
def test_param_grads_variance(cid):
    """d / d variance = 10 inv_s sum(rows) inside the clip range of exp(10 variance), exactly nothing added where the clip is active"""
    e = _Entries()
    e.variance(cid)
    e.launch_and_check()


def test_param_grads_full_launch_and_refusal():
    """AC_PG_MAX_ENTRIES entries of the three kinds in shuffled order, one launch: the blk0 table at its full length; one entry more is refused"""
    from avatarcraft_amd import nsr_ops
    e = _Entries()
    for cid, off, pad in (("r65c37", 0, 0), ("r3c300", 7, 2), ("r5c257", 0, 3), ("r1c1", 1, 1), ("r16c64", 0, 0)):
        e.weight_norm(cid, off, pad)
    for rows, stride in ((1, 36), (16, 1), (300, 36), (300, 1)):
        e.add(rows, stride)
    for cid in ("v0.6-n5000", "v1.5-n255", "v-0.9-n1"):
        e.variance(cid)
    assert len(e.entries) == SC.PG_MAX_ENTRIES
    e.launch_and_check(order=list(np.random.RandomState(3).permutation(SC.PG_MAX_ENTRIES)))
    before = [(t[7].clone(), None if t[8] is None else t[8].clone()) for t in e.entries]
    with pytest.raises(RuntimeError, match="param_grads"):
        nsr_ops.param_grads(e.entries + [e.entries[0]], torch.device(DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(t[7], b[0]) and (t[8] is None or torch.equal(t[8], b[1])) for t, b in zip(e.entries, before))


def test_weight_norm_all_under_autograd():
    """the operator the model uses: every shape in one launch each way, one layer left out of the loss (its upstream gradient is None)"""
    from avatarcraft_amd import nsr_ops
    ids = [i for i in sorted(WN) if not i.startswith("full")]
    layers = [SC.wn_layer(*WN[i]) for i in ids]
    mods = [types.SimpleNamespace(weight_v=dev(l["v"], True), weight_g=dev(l["g"], True)) for l in layers]
    Ws = nsr_ops.weight_norm_all(mods)
    skip = 2
    sum((W * dev(l["gw"])).sum() for k, (W, l) in enumerate(zip(Ws, layers)) if k != skip).backward()
    for k, (i, l, m, W) in enumerate(zip(ids, layers, mods, Ws)):
        ref = SC.wn_eval(l, F64)
        check("weight_norm", i, {"w": W}, ref, names=["w"])
        if k == skip:
            assert all(g is None or float(g.abs().max()) == 0.0 for g in (m.weight_v.grad, m.weight_g.grad))
        else:
            check("weight_norm", i, {"g_v": m.weight_v.grad, "g_g": m.weight_g.grad}, ref, names=["g_v", "g_g"])


# ---- sds_upstream --------------------------------------------------------------------------------------------------------------------------------
SDS = SC.sds_cases()


@pytest.mark.parametrize("cid", sorted(SDS))
def test_sds_upstream_matches_float64_autograd(cid):
    from avatarcraft_amd import nsr_ops, _lib as L
    c = SDS[cid]
    inp = SC.sds_inputs(c)
    ws, gt, N = dev(inp["ws"]), dev(inp["gt"]), c["N"]
    g, loss = nsr_ops.sds_upstream(ws, gt, inp["scale"])
    ref = SC.sds_eval(c, inp, F64)
    check("sds_upstream", cid, {"g_ws": g, "loss": loss}, ref)
    outside = (inp["ws"] < 0) | (inp["ws"] > 1)
    assert float(g.cpu()[outside].abs().max() if outside.any() else 0.0) == 0.0                      # the clamp passes nothing outside [0, 1] ...
    at_edge = ((inp["ws"] == 0) | (inp["ws"] == 1)) & (inp["gt"].clamp(0, 1) != inp["ws"])
    assert (g.cpu()[at_edge] != 0).all()                                                             # ... and passes at exactly 0 and 1
    # want_grad=False: only the loss; the loss pointer alone and the gradient pointer alone each work, neither is refused
    g0, loss0 = nsr_ops.sds_upstream(ws, gt, inp["scale"], want_grad=False)
    assert g0 is None and same_bits([loss0], [loss])
    buf = torch.full((N + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    L.check(L.lib().ac_sds_upstream(ws.data_ptr(), gt.data_ptr(), N, float(inp["scale"]), buf.data_ptr(), None, L.current_stream(torch.device(DEV))), "sds_upstream")
    torch.cuda.synchronize()
    assert same_bits([buf[:N]], [g]) and float((buf[N:] - SENTINEL).abs().max()) == 0.0
    assert L.lib().ac_sds_upstream(ws.data_ptr(), gt.data_ptr(), N, float(inp["scale"]), None, None, L.current_stream(torch.device(DEV))) != 0
