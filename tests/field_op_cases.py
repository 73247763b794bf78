"""Cases and restatements for the two arithmetic-heavy training operators, nsr_ops.sdf_stencil (csrc/sdf_stencil_train.hip, hash_stencil.hip) and
nsr_ops.color_mlp (csrc/color_train.hip).  GPU tier: tests/test_gpu_field_ops.py, CPU tier: tests/test_field_ops_host.py, bounds:
tests/golden/make_field_op_bounds.py -> tests/golden/field_op_bounds.json.  The rule and its constants are those of tests/step_op_cases.py.

Plain torch on the CPU, no GPU import.  The restatements are the reference's own lines -- the hash encoding (hashencoder.cu:55-70, 121-166, default
layout: 16 levels, 2 features, base 16, log2 size 19), forward_sdf (models/instant_nsr.py:627-642), finite_difference_normals_approximator (:687-704) and
forward_color without view directions (:644-663) -- written to run in the dtype of their inputs: float32 against float64 gives err32 per tensor.

A second mode of the same restatements, "K", is a model of the ROUNDING the kernels declare in their headers (float32 throughout):
  * softplus(beta = 100) and its derivative from the 128-piece cubic of tools/gen_softplus_table.fit(), the backward being the cubic's own derivative;
  * SDF backward: dinp = W1[:, 3:]^T d1 as a three-term bf16 split (weights rounded to nearest, d1 truncated: split8_bf16), layer 1 of the six offset
    evaluations recomputed as the centre's plus a three-term split of W1[:, 3:] (fe - fe0) (sdf_l1_delta, differences truncated); dW1 += d1 inp^T is
    a float32 product in the stand-alone operator (the bf16 form belongs to the saved-feature variant, which only ac_render_core_backward reaches:
    SdfLayer1's dw1, used by tests/core_backward_cases.py);
  * colour backward: layer 3 of the recomputation, dh1 = Wc2^T dh2 and dinp = Wc1^T dh1 as three-term splits, both factors rounded to nearest;
  * every (sample, point, corner) contribution to the table gradient rounded to 16 / 17 explicit mantissa bits (rec_round) and summed exactly (the
    64-bit fixed-point grid lies 2^-40 below the level's largest record at these sizes), one rounding to float32 at the end.
It reproduces no lane layout and no summation order.  errK = max|K - f64|; the GPU tier allows FACTOR * max(err32, errK) + FLOOR * max|f64|.

Every input is drawn in float64 and rounded to float32 once; each quantity has a generator of its own, seeded by the case without its row count and
filled row by row, so a larger launch starts with the smaller one's rows.  SDF points are drawn with a deterministic rejection rule (twice the rows,
the first B that pass): no position of the stencil within 2^-10 cells of a cell face on any level (float32 places pos <= 2048 within 5e-4, so both
precisions and both roundings of u * scale + 0.5 see the same cell; the derivative of a trilinear interpolant jumps at a face), and no x_k +- eps
exactly on +-bound in float32.  Colour rows are rejected where a hidden pre-activation has |sum w h| < 2^-12 sum |w h| in float64 (64 times float32's
worst rounding of a 64-term dot product: no ReLU gate differs between the precisions)."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from tests.step_op_cases import FACTOR, FLOOR, GMAX_MIN, F32, f32, _rs, _t       # noqa: F401  (the rule's constants live there)
from tests.common import load_golden, make_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, EPS = f32(1.6), f32(0.005)
LEVELS, BASE = 16, 16
FACE_MARGIN = 2.0 ** -10
GATE_MARGIN = 2.0 ** -12
K = "K"                                                    # the declared-arithmetic mode
SPECIAL_FROM = 40                                          # candidate row from which the edge rows of the SDF points are placed


def bound_of(err32, errK, max64):
    return FACTOR * max(err32, errK) + FLOOR * max64


# ---- the hash grid's layout ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params():
    return load_golden("nsr_params.npz")


@functools.lru_cache(maxsize=None)
def layout():
    """per level: scale (the float32 value of exp2f(level * S) * H - 1), entries, hashed?, first row -- hashencoder.cu:55-70, 121-123"""
    p = params()
    offsets = p["offsets"].astype(np.int64)
    S = F32(np.log2(float(p["per_level_scale"])))
    lv = []
    for l in range(LEVELS):
        scale = F32(2.0 ** float(F32(l) * S)) * F32(BASE) - F32(1.0)       # a correctly rounded exp2f (numpy's float32 exp2 is 1 ulp off on five levels)
        res = int(np.ceil(scale)) + 1
        size = int(offsets[l + 1] - offsets[l])
        stride = 1
        for _ in range(3):
            if stride <= size:
                stride *= res + 1
        lv.append(dict(scale=float(scale), res=res, size=size, hashed=stride > size, offset=int(offsets[l])))
    return lv


def table_offsets():
    return params()["offsets"].astype(np.int64)


def stencil_points(x, clamp_passes_gradient=False, clamp=True):
    """[B,3] -> [7,B,3]: x, then clamp(x +- eps e_k, -bound, bound) in the order +x, -x, +y, -y, +z, -z (models/instant_nsr.py:690-702)"""
    pts = [x]
    for k in range(3):
        for sgn in (1.0, -1.0):
            e = torch.zeros(3, dtype=x.dtype)
            e[k] = sgn * EPS
            raw = x + e
            cl = raw.clamp(-BOUND, BOUND)
            pts.append(raw if not clamp else raw + (cl - raw).detach() if clamp_passes_gradient else cl)
    return torch.stack(pts)


def cell_positions(pts, scale_mode="f64"):
    """pos = u * scale + 0.5 of numpy points [...,3] on every level -> [...,16,3].  f64: exact to 1e-13; f32_fma: float32 u, one rounding of the
    product-and-sum (the kernels' fma); f32_mul_add: two roundings (torch)"""
    scale = np.array([lv["scale"] for lv in layout()])
    if scale_mode == "f64":
        u = (pts.astype(np.float64) + BOUND) / (2.0 * BOUND)
        return u[..., None, :] * scale[:, None] + 0.5
    u = ((pts.astype(F32) + F32(BOUND)) / F32(2.0 * BOUND)).astype(F32)
    if scale_mode == "f32_fma":
        return (u.astype(np.float64)[..., None, :] * scale[:, None] + 0.5).astype(F32)
    return (u[..., None, :] * scale.astype(F32)[:, None]).astype(F32) + F32(0.5)


def corner_rows(cell):
    """cells [...,16,3] int64 -> rows of the whole table [...,16,8] of the cell's corners, corner bit d = axis d (hashencoder.cu:55-70, 142-157)"""
    out = np.empty(cell.shape[:-1] + (8,), np.int64)
    for l, lv in enumerate(layout()):
        for idx in range(8):
            c = [cell[..., l, d] + ((idx >> d) & 1) for d in range(3)]
            if lv["hashed"]:
                i = (c[0] ^ ((c[1] * 2654435761) & 0xffffffff) ^ ((c[2] * 805459861) & 0xffffffff)) & 0xffffffff
            else:
                i = (c[0] + c[1] * (lv["res"] + 1) + c[2] * (lv["res"] + 1) ** 2) & 0xffffffff
            out[..., l, idx] = lv["offset"] + i % lv["size"]
    return out


def geometry(x32):
    """the stencil's cells and the compact leaf of one batch: cell [7,B,16,3], rows [R] (the touched table rows, sorted), slot [7,B,16,8] into them,
    seg [17] (level l owns rows[seg[l]:seg[l + 1]])"""
    pts = stencil_points(torch.from_numpy(np.ascontiguousarray(x32)).double()).numpy()
    cell = np.floor(cell_positions(pts)).astype(np.int64)
    glob = corner_rows(cell)
    rows, slot = np.unique(glob, return_inverse=True)
    return dict(cell=torch.from_numpy(cell), rows=rows, slot=torch.from_numpy(slot.reshape(glob.shape)), seg=np.searchsorted(rows, table_offsets()))


_BITS = torch.tensor([[(i >> d) & 1 for i in range(8)] for d in range(3)], dtype=torch.bool)


def encode(pts, geo, leaf):
    """[7,B,3] -> features [7,B,32] (level-major, 2 per level) and the trilinear weights [7,B,16,8], in the dtype of pts; leaf [R,2] = the touched rows"""
    scale = torch.tensor([lv["scale"] for lv in layout()], dtype=pts.dtype)
    u = (pts + BOUND) / (2.0 * BOUND)
    fr = (u[:, :, None, :] * scale[:, None] + 0.5) - geo["cell"].to(pts.dtype)
    w = 1.0
    for d in range(3):
        f = fr[..., d:d + 1]
        w = w * torch.where(_BITS[d], f, 1.0 - f)
    feat = (w[..., None] * leaf[geo["slot"]]).sum(-2)
    return feat.reshape(pts.shape[0], pts.shape[1], 2 * LEVELS), w


# ---- the declared arithmetic ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def softplus_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_softplus_table
    finally:
        sys.path.pop(0)
    return torch.from_numpy(gen_softplus_table.fit())


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


class TableSoftplus(torch.autograd.Function):
    """softplus_100 = max(x, 0) + q(fract(a4)), a4 = min(|400 x|, 128), q the cubic of row int(a4); backward: the cubic's own derivative"""

    @staticmethod
    def forward(ctx, x):
        tab = softplus_table()
        a4 = (x * 400.0).abs().clamp(max=128.0)
        c = tab[a4.long()]
        v = a4 - a4.floor()
        q = _fma(_fma(_fma(c[..., 3], v, c[..., 2]), v, c[..., 1]), v, c[..., 0])
        dq = _fma(_fma(3.0 * c[..., 3], v, 2.0 * c[..., 2]), v, c[..., 1])
        pos = x > 0
        ctx.save_for_backward(pos.float() + torch.where(pos, 400.0, -400.0) * dq)
        return _fma(torch.full_like(x, 0.5), x.abs(), _fma(torch.full_like(x, 0.5), x, q))

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


def split_bf16(v, rounding):
    """float32 -> (hi, lo) as float32 values; "rn": both parts rounded to nearest even, "trunc": the top 16 bits of v and of v - hi (split8_bf16)"""
    if rounding == "rn":
        hi = v.bfloat16().float()
        return hi, (v - hi).bfloat16().float()
    top = lambda t: (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hi = top(v)
    return hi, top(v - hi)


def split_mm(act, W, rounding, drop_lo=False):
    """act [B,K] x W [N,K]^T with both factors split hi + lo, the lo x lo term dropped, float32 sums (drop_lo: the hi x hi term alone -- a mutant)"""
    ah, al = split_bf16(act, rounding)
    wh, wl = split_bf16(W, "rn")
    return ah @ wh.T if drop_lo else ah @ wh.T + ah @ wl.T + al @ wh.T


class DeclaredLinear(torch.autograd.Function):
    """y = x W^T.  fwd / bwd: None = a float32 product, "rn" / "trunc" = the three-term split with the activations rounded that way; the weight
    gradient is always a float32 product"""

    @staticmethod
    def forward(ctx, x, W, fwd, bwd, drop_lo):
        ctx.save_for_backward(x, W)
        ctx.bwd, ctx.drop_lo = bwd, drop_lo
        return x @ W.T if fwd is None else split_mm(x, W, fwd)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        gx = g @ W if ctx.bwd is None else split_mm(g, W.T.contiguous(), ctx.bwd, ctx.drop_lo)
        return gx, g.T @ x, None, None, None


class SdfLayer1(torch.autograd.Function):
    """a = [p, feat] W1^T + b1 with the backward of sdf_stencil_bwd_kernel: d p through W1[:, :3] in float32, d feat as the truncated three-term split,
    d W1 and d b1 float32.  value: the pre-activation the backward recomputes for an offset evaluation (sdf_l1_delta), in place of the plain product.
    dw1: None = d W1 += d1 inp^T as a float32 product (the stand-alone operator); "split" = the saved-feature variant's (sdf_stencil_bwd_kernel<SAVED =
    true>, reached through ac_render_core_backward alone): d1 and inp = [p, feat, 1] split hi + lo, each part rounded to nearest, hi hi + lo hi + hi lo
    with float32 sums, d b1 the column of ones of that product; "hi" = the hi x hi term alone (a mutant)"""

    @staticmethod
    def forward(ctx, p, feat, W1, b1, value, drop_lo, dw1=None):
        ctx.save_for_backward(p, feat, W1)
        ctx.drop_lo, ctx.dw1 = drop_lo, dw1
        return p @ W1[:, :3].T + feat @ W1[:, 3:].T + b1 if value is None else value.clone()

    @staticmethod
    def backward(ctx, g):
        p, feat, W1 = ctx.saved_tensors
        inp = torch.cat([p, feat], -1)
        if ctx.dw1 is None:
            gW, gb = g.T @ inp, g.sum(0)
        else:
            (dh, dl), (ih, il) = split_bf16(g, "rn"), split_bf16(inp, "rn")
            gW, gb = (dh.T @ ih, dh.sum(0)) if ctx.dw1 == "hi" else (dh.T @ ih + dl.T @ ih + dh.T @ il, dh.sum(0) + dl.sum(0))
        return (g @ W1[:, :3], split_mm(g, W1[:, 3:].T.contiguous(), "trunc", ctx.drop_lo), gW, gb, None, None, None)


def round_record(v, drop):
    """rec_round of table_scatter.hpp: to nearest at bit `drop` of the float32 pattern"""
    b = np.ascontiguousarray(v, F32).view(np.uint32)
    return ((b + np.uint32(1 << (drop - 1))) & np.uint32(~((1 << drop) - 1) & 0xffffffff)).view(F32)


def declared_table_gradient(w, gfeat, geo):
    """contributions w [7,B,16,8] * gfeat [7,B,16,2] as float32 products, rounded as records (channel 0: 16 explicit bits, channel 1: 17), summed
    exactly per touched row, rounded to float32 once -> [R,2]"""
    c = w.detach().numpy().astype(F32)[..., None] * gfeat.detach().numpy().astype(F32).reshape(w.shape[0], w.shape[1], LEVELS, 1, 2)
    c = np.stack([round_record(c[..., 0], 7), round_record(c[..., 1], 6)], -1).astype(np.float64)
    out = np.zeros((len(geo["rows"]), 2))
    np.add.at(out, geo["slot"].numpy().reshape(-1), c.reshape(-1, 2))
    return out.astype(F32).astype(np.float64)


# ---- restatements --------------------------------------------------------------------------------------------------------------------------------------
def fd_gradient(sd, pts, by_clamped_distance=False):
    """sd [6,B] -> [B,3]: 0.5 (s+ - s-) / eps, always by eps (models/instant_nsr.py:704)"""
    cols = []
    for k in range(3):
        den = (0.5 * (pts[1 + 2 * k, :, k] - pts[2 + 2 * k, :, k])).detach() if by_clamped_distance else EPS
        cols.append(0.5 * (sd[2 * k] - sd[2 * k + 1]) / den)
    return torch.stack(cols, -1)


def sdf_query_ref(pts, feat, W1, b1, W2, b2, act=None, mutant=None):
    """forward_sdf on the 7 points (models/instant_nsr.py:627-642) and the finite-difference gradient (:687-704) -> out16 [B,16], gradient [B,3]"""
    act = act or (lambda a: F.softplus(a, beta=100))
    o = act(torch.cat([pts, feat], -1) @ W1.T + b1) @ W2.T + b2
    return o[0], fd_gradient(o[1:, :, 0], pts, mutant == "div_clamped")


def sdf_query_declared(pts, feat, W1, b1, W2, b2, drop_lo=False, dw1=None):
    """the arithmetic of sdf_stencil_bwd_kernel: the centre's layer 1 in float32, the six offset evaluations' as corrections of it (dw1: SdfLayer1)"""
    a0 = SdfLayer1.apply(pts[0], feat[0], W1, b1, None, drop_lo, dw1)
    out16 = TableSoftplus.apply(a0) @ W2.T + b2
    sd = []
    with torch.no_grad():
        W1d = W1.detach()
    for e in range(1, 7):
        k = (e - 1) >> 1
        with torch.no_grad():
            value = a0 + split_mm(feat[e] - feat[0], W1d[:, 3:], "trunc") + (pts[e, :, k] - pts[0, :, k])[:, None] * W1d[:, k]
        a = SdfLayer1.apply(pts[e], feat[e], W1, b1, value, drop_lo, dw1)
        sd.append((TableSoftplus.apply(a) * W2[0]).sum(-1) + b2[0])
    return out16, fd_gradient(torch.stack(sd), pts)


class ReluMaskedBy(torch.autograd.Function):
    """relu(a) whose backward takes its mask from another tensor (a mutant)"""

    @staticmethod
    def forward(ctx, a, other):
        ctx.save_for_backward(other)
        return a.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        return g * (ctx.saved_tensors[0] > 0), None


def color_ref(x, n, out16, Wc1, Wc2, Wc3, declared=False, mutant=None):
    """forward_color without view directions (models/instant_nsr.py:644-663): cat[x, n, out16[:, 1:]] -> ReLU -> ReLU -> sigmoid.  declared: the
    arithmetic of color_bwd_kernel (layers 1 and 2 forward in float32: they decide the ReLU masks)"""
    h = torch.cat([x, n, out16[:, 1:]], -1)
    lin = (lambda t, W, fwd, bwd: DeclaredLinear.apply(t, W, fwd, bwd, False)) if declared else (lambda t, W, fwd, bwd: t @ W.T)
    a1 = lin(h, Wc1, None, "rn")
    a2 = lin(F.relu(a1), Wc2, None, "rn")
    h2 = ReluMaskedBy.apply(a2, a1) if mutant == "relu2_from_l1" else F.relu(a2)
    return torch.sigmoid(lin(h2, Wc3, "rn", None))


# ---- weights ---------------------------------------------------------------------------------------------------------------------------------------------
SDF_W, COLOR_W = ("W1", "b1", "W2", "b2"), ("Wc1", "Wc2", "Wc3")
WEIGHTS = ("golden", "drawn")


@functools.lru_cache(maxsize=None)
def table_of(kind):
    """float32 [6119857, 2]; golden: make_table of the stored seed; drawn: a stream of its own at twice the golden amplitudes (every level non-zero)"""
    p = params()
    if kind == "golden":
        return make_table(int(p["offsets"][-1]), seed=int(p["table_seed"]), offsets=p["offsets"], level_amp=p["level_amp"])
    amp = np.repeat(2.0 * np.asarray(p["level_amp"], np.float64), np.diff(table_offsets()))
    return (_rs("field", "drawn", "table").uniform(-1.0, 1.0, size=(int(p["offsets"][-1]), 2)) * amp[:, None]).astype(F32)


@functools.lru_cache(maxsize=None)
def weights_of(kind):
    """effective matrices as float32 tensors.  drawn: scaled so that the layer-1 pre-activations of the SDF query reach the knee of the softplus, the
    end of its table and both signs on >= 5 % of (sample, unit) pairs each (tests/test_field_ops_host.py)"""
    if kind == "golden":
        return {k: torch.from_numpy(params()[k].copy()) for k in SDF_W + COLOR_W}
    n = lambda name, shape, s: _t(_rs("field", "drawn", name).normal(0.0, s, shape))
    W1 = torch.cat([n("W1x", (64, 3), 0.06), n("W1f", (64, 32), 0.6)], -1)
    return dict(W1=W1, b1=n("b1", (64,), 0.1), W2=n("W2", (16, 64), 0.2), b2=n("b2", (16,), 0.1), Wc1=n("Wc1", (64, 21), 0.4), Wc2=n("Wc2", (64, 64), 0.2),
                Wc3=n("Wc3", (3, 64), 0.3))


# ---- sdf_stencil: cases and inputs ---------------------------------------------------------------------------------------------------------------------
B_LIST = [1, 15, 16, 17, 63, 65, 1000]
SMALL_LAUNCH = 37
SDF_LOSSES = {"all": ("out16", "gradient"), "sdf16": ("out16",), "normal": ("gradient",)}
TABLE_TENSORS = tuple(f"g_table_L{l:02d}" for l in range(LEVELS))
SDF_TENSORS = ("out16", "gradient", "g_W1", "g_b1", "g_W2", "g_b2") + TABLE_TENSORS


def large_launch(cu_count):
    """the second trip of every persistent grid: 12 tiles of 16 rows per CU is the colour forward's residency, the other kernels hold fewer"""
    return 16 * 12 * int(cu_count) + 5


def sdf_case(B, weights="golden", loss="all", gx=False):
    return dict(B=B, weights=weights, loss=loss, gx=gx)


def sdf_cases():
    cases = {}

    def add(c):
        cases["{weights}-{loss}-{g}-b{B}".format(g="gx" if c["gx"] else "nogx", **c)] = c
    for B in B_LIST:
        add(sdf_case(B))
    for B in (17, 1000):
        add(sdf_case(B, "drawn"))
    for loss in ("sdf16", "normal"):
        add(sdf_case(65, loss=loss))
    for B in (1, 17, 1000):
        for wk in WEIGHTS:
            add(sdf_case(B, wk, gx=True))
    return cases


def sdf_tensors(c):
    return SDF_TENSORS + (("g_x",) if c["gx"] else ())


def _key(fam, c):
    return (fam,) + tuple(v for k, v in sorted(c.items()) if k != "B")


def sdf_rows_pass(x32):
    """the two rejection rules, per row of float32 points [n,3]"""
    x32 = np.ascontiguousarray(x32, F32)
    x = x32.astype(np.float64)
    offs = np.stack([x, np.clip(x + EPS, -BOUND, BOUND), np.clip(x - EPS, -BOUND, BOUND)], 1)                # [n, 3 offsets, 3 axes]
    pos = cell_positions(offs)                                                                                  # [n, 3, 16, 3]
    faces = (np.abs(pos - np.round(pos)) < FACE_MARGIN).any(axis=(1, 2, 3))
    up, dn, b = x32 + F32(EPS), x32 - F32(EPS), F32(BOUND)
    edge = ((up == b) | (up == -b) | (dn == b) | (dn == -b)).any(-1)
    return ~faces & ~edge


SDF_SPECIALS = ("on_plus_bound", "on_minus_bound", "near_plus_bound", "near_minus_bound", "corner")


def _special(row, name):
    row = row.copy()
    if name == "on_plus_bound":
        row[0] = BOUND
    elif name == "on_minus_bound":
        row[1] = -BOUND
    elif name == "near_plus_bound":
        row[2] = BOUND - 0.5 * EPS                         # x + eps is clamped
    elif name == "near_minus_bound":
        row[0] = -BOUND + EPS / 3.0                        # x - eps is clamped
    else:
        row[:] = [BOUND, -BOUND, BOUND]
    return row


def sdf_points(key, B):
    """-> (x float32 [B,3], {special: row index}).  Candidates are walked in order; from candidate SPECIAL_FROM on, the next edge row still to be
    placed is written over the candidate (and tried again on the next one if it is rejected)"""
    cand = _rs(*key, "x").uniform(-BOUND, BOUND, (2 * B, 3))
    todo, where = list(SDF_SPECIALS), {}
    ok = sdf_rows_pass(cand.astype(F32))
    keep = []
    for i in range(len(cand)):
        if len(keep) == B:
            break
        if i >= SPECIAL_FROM and todo:
            cand[i] = _special(cand[i], todo[0])
            if sdf_rows_pass(cand[i:i + 1].astype(F32))[0]:
                where[todo.pop(0)] = len(keep)
                keep.append(i)
        elif ok[i]:
            keep.append(i)
    assert len(keep) == B, (key, B, len(keep))
    return cand[keep].astype(F32), where


def sdf_inputs(c, rows=None):
    """float32 CPU tensors of one case; rows: a slice of the launch's rows to keep (the restatement of the last rows of a large launch)"""
    key, B = _key("sdf", c), c["B"]
    x, where = sdf_points(key, B)
    up = {"out16": _t(_rs(*key, "u16").normal(size=(B, 16))), "gradient": _t(_rs(*key, "u3").normal(size=(B, 3)))}
    x = torch.from_numpy(x)
    if rows is not None:
        x, up = x[rows].contiguous(), {k: v[rows].contiguous() for k, v in up.items()}
    return dict(x=x, up=up, where=where)


def sdf_loss(c, out16, gradient, up, mutant=None):
    out = {"out16": out16, "gradient": gradient}
    if mutant == "pad_lanes":                              # the padding lanes of the last tile re-read the last row: counted, it weighs 1 + (16 - B mod 16)
        up = {k: torch.cat([v[:-1], v[-1:] * (1 + (16 - len(v) % 16) % 16)]) for k, v in up.items()}
    return sum((out[k] * up[k].to(out[k].dtype)).sum() for k in SDF_LOSSES[c["loss"]])


def _per_level(g_rows, geo):
    return {name: g_rows[geo["seg"][l]:geo["seg"][l + 1]] for l, name in enumerate(TABLE_TENSORS)}


def _np64(t):
    return t.detach().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


def sdf_eval(c, inp, mode, geo=None, mutant=None):
    """the restatement in float32 / float64, or the declared arithmetic (mode K): {tensor: float64 array}; the table gradient per level, on the touched
    rows geo["rows"] in their order"""
    geo = geo or geometry(inp["x"].numpy())
    dt = torch.float32 if mode == K else mode
    Wt = weights_of(c["weights"])
    W = [Wt[k].detach().clone().to(dt).requires_grad_(True) for k in SDF_W]
    x = inp["x"].detach().clone().to(dt).requires_grad_(c["gx"])
    leaf = torch.from_numpy(table_of(c["weights"])[geo["rows"]]).to(dt).requires_grad_(mode != K)
    pts = stencil_points(x, mutant == "clamp_passes")
    feat, w = encode(pts, geo, leaf)
    if mutant == "no_clamp":                               # the offset point leaves the cube, where the encoder returns zeros (hashencoder.cu:95-119)
        raw = stencil_points(x, clamp=False)
        feat, pts = feat * ((raw.detach().abs() <= BOUND).all(-1, keepdim=True)).to(dt), raw
    if mode != K:
        out16, gradient = sdf_query_ref(pts, feat, *W, mutant=mutant)
        sdf_loss(c, out16, gradient, inp["up"], mutant).backward()
        g_rows = _np64(leaf.grad)
    else:
        with torch.no_grad():                              # the forward kernel: float32 products, the table softplus
            out16, gradient = sdf_query_ref(pts, feat, *W, act=TableSoftplus.apply)
        pts_d, feat_d = pts.detach().requires_grad_(c["gx"]), feat.detach().requires_grad_(True)
        sdf_loss(c, *sdf_query_declared(pts_d, feat_d, *W, drop_lo=mutant == "drop_lo"), inp["up"], mutant).backward()
        g_rows = declared_table_gradient(w, feat_d.grad, geo)
        if c["gx"]:
            torch.autograd.backward([pts, feat], [pts_d.grad, feat_d.grad])
    res = dict(out16=_np64(out16), gradient=_np64(gradient), **{"g_" + k: _np64(t.grad) for k, t in zip(SDF_W, W)}, **_per_level(g_rows, geo))
    if c["gx"]:
        res["g_x"] = _np64(x.grad)
    return res


# ---- color_mlp: cases and inputs -----------------------------------------------------------------------------------------------------------------------
COLOR_TENSORS = ("rgb", "g_normal", "g_sdf16", "g_Wc1", "g_Wc2", "g_Wc3")


def color_case(B, weights="golden", up="all"):
    return dict(B=B, weights=weights, up=up)


def color_cases():
    cases = {}

    def add(c):
        cases["{weights}-{up}-b{B}".format(**c)] = c
    for B in B_LIST:
        add(color_case(B))
    for B in (17, 1000):
        add(color_case(B, "drawn"))
    add(color_case(65, up="every_second_row_zero"))
    return cases


def color_rows_pass(x, n, o, Wt, margin=GATE_MARGIN):
    """float64 arrays: no hidden pre-activation of layer 1 or 2 within margin (GATE_MARGIN) of its terms' absolute sum"""
    h = np.concatenate([x, n, o[:, 1:]], -1)
    W1, W2 = Wt["Wc1"].double().numpy(), Wt["Wc2"].double().numpy()
    a1, s1 = h @ W1.T, np.abs(h) @ np.abs(W1).T
    h1 = np.maximum(a1, 0.0)
    a2, s2 = h1 @ W2.T, h1 @ np.abs(W2).T
    return ~((np.abs(a1) < margin * s1).any(-1) | (np.abs(a2) < margin * s2).any(-1))


ZERO_NORMAL_FROM = 3                                       # candidate row from which the row with an all-zero normal is placed


def color_inputs(c, rows=None):
    key, B, Wt = _key("color", c), c["B"], weights_of(c["weights"])
    m = 2 * B
    x = _rs(*key, "x").uniform(-BOUND, BOUND, (m, 3))
    d = _rs(*key, "nd").normal(size=(m, 3))
    n = d / np.linalg.norm(d, axis=-1, keepdims=True) * _rs(*key, "nl").uniform(0.1, 1.0, (m, 1))
    o = _rs(*key, "o").normal(0.0, 0.3, (m, 16))
    r = lambda a: a.astype(F32).astype(np.float64)         # the rule is evaluated on the float32 values both sides see
    ok = color_rows_pass(r(x), r(n), r(o), Wt)
    keep, zero_row = [], None
    for i in range(m):
        if len(keep) == B:
            break
        if i >= ZERO_NORMAL_FROM and zero_row is None:
            n[i] = 0.0
            if color_rows_pass(r(x[i:i + 1]), r(n[i:i + 1]), r(o[i:i + 1]), Wt)[0]:
                zero_row = len(keep)
                keep.append(i)
        elif ok[i]:
            keep.append(i)
    assert len(keep) == B, (key, B, len(keep))
    up = _rs(*key, "up").normal(size=(B, 3))
    if c["up"] == "every_second_row_zero":
        up[1::2] = 0.0
    inp = dict(x=_t(x[keep]), normal=_t(n[keep]), out16=_t(o[keep]), up=_t(up), zero_row=zero_row)
    if rows is not None:
        inp.update({k: inp[k][rows].contiguous() for k in ("x", "normal", "out16", "up")})
    return inp


def color_eval(c, inp, mode, mutant=None):
    dt = torch.float32 if mode == K else mode
    Wt = weights_of(c["weights"])
    W = [Wt[k].detach().clone().to(dt).requires_grad_(True) for k in COLOR_W]
    n, o = (inp[k].detach().clone().to(dt).requires_grad_(True) for k in ("normal", "out16"))
    x = inp["x"].to(dt)
    rgb = color_ref(x, n, o, *W, declared=mode == K, mutant=mutant)
    (rgb * inp["up"].to(dt)).sum().backward()
    if mode == K:
        with torch.no_grad():                              # the forward kernel's products are float32
            rgb = color_ref(x, n, o, *W)
    return dict(rgb=_np64(rgb), g_normal=_np64(n.grad), g_sdf16=_np64(o.grad), **{"g_" + k: _np64(t.grad) for k, t in zip(COLOR_W, W)})


# ---- everything the bounds file records ----------------------------------------------------------------------------------------------------------------
GMAX_KEY = {"sdf_stencil": "g_W1", "color_mlp": "g_Wc1"}


def families():
    """family -> (cases, evaluate(case, mode) -> {tensor: float64 array}, tensors(case))"""
    def sdf(c, modes):
        inp = sdf_inputs(c)
        geo = geometry(inp["x"].numpy())
        return [sdf_eval(c, inp, m, geo) for m in modes]

    def color(c, modes):
        inp = color_inputs(c)
        return [color_eval(c, inp, m) for m in modes]
    return {"sdf_stencil": (sdf_cases(), sdf, sdf_tensors), "color_mlp": (color_cases(), color, lambda c: COLOR_TENSORS)}


def measure3(r32, rK, r64):
    """{tensor: [err32, errK, max|f64|]} of one case evaluated in the three modes"""
    rec = {}
    for k in sorted(r64):
        a, b, ref = r32[k], rK[k], r64[k]
        assert a.shape == ref.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(ref).all(), k
        e = lambda t: float(np.abs(t - ref).max()) if ref.size else 0.0
        rec[k] = [e(a), e(b), float(np.abs(ref).max()) if ref.size else 0.0]
    return rec
