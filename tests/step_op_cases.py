"""Cases and float64 restatements for the small differentiable operators around the MLPs (GPU tier: tests/test_gpu_step_ops.py, CPU tier:
tests/test_step_ops_host.py, bounds: tests/golden/make_step_op_bounds.py -> tests/golden/step_op_bounds.json).

Plain torch on the CPU, no GPU import.  The restatements are the reference's own lines (models/instant_nsr.py:215, 222-263, 266-272, 290-294, 35-45;
stylize.py:183-193; torch.nn.utils.weight_norm), written to run in whatever dtype their inputs have: once in float32 and once in float64 they give the
reference formulation's own rounding error err32 = max|f32 - f64| per tensor, from which the GPU tier's bound 4 * err32 + 2^-21 * max|f64| is formed.

Every input is drawn in float64 and rounded to float32 ONCE; both sides see those float32 values.  Every quantity has a generator of its own, seeded
by the case's parameters without the row count and filled row by row, so a larger launch of the same family starts with the smaller one's rows.
Gradients come from one scalar loss with fixed random upstream weights on every differentiable output."""
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
FACTOR = 4.0                           # kernel error allowed per tensor: FACTOR * err32 + FLOOR * max|f64|
FLOOR = 2.0 ** -21                     # four fp32 ulps of the largest entry (err32 can be zero by luck)
GMAX_MIN = 1e-2                        # every gradient case: the float64 max|g| is at least this (no silently degenerate case)


def f32(x):
    return float(F32(x))


def _rs(*key):
    return np.random.RandomState(zlib.crc32("/".join(str(k) for k in key).encode()))


def _t(a):
    """float64 values -> the float32 tensor both sides see"""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).astype(F32)))


def bound_of(err32, max64):
    return FACTOR * err32 + FLOOR * max64


def cube_near_far(ro, rd, bound):
    """near_far_from_bound (cube) in fp32, the renderers' arithmetic (pinned by tests/golden/rays.npz through the render tests)"""
    from tests.test_long_posed_cpu import cube_near_far as nf
    return nf(ro, rd, bound)


# ---- restatements --------------------------------------------------------------------------------------------------------------------------------
def neus_alpha_ref(sdf, true_cos, deltas, inv_s, car, softplus=None):
    """models/instant_nsr.py:222-243; sdf, true_cos, deltas of one shape, inv_s broadcastable, car a Python float (softplus: another evaluation of
    softplus(beta = 100) -- the kernels' table cubic, for a model of their declared arithmetic)"""
    softplus = softplus or (lambda a: F.softplus(a, beta=100))
    iter_cos = -(softplus(-true_cos * 0.5 + 0.5) * (1.0 - car) + softplus(-true_cos) * car)
    next_sdf = sdf + iter_cos * deltas * 0.5
    prev_sdf = sdf - iter_cos * deltas * 0.5
    prev_cdf, next_cdf = torch.sigmoid(prev_sdf * inv_s), torch.sigmoid(next_sdf * inv_s)
    return ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).clip(0.0, 1.0)


def composite_from_alpha(alpha, color, z, near, far, bg, normal=None):
    """models/instant_nsr.py:250-263, 290-294: the compositing half, from alpha [N,T] on; near / far [N]"""
    N = alpha.shape[0]
    weights = alpha * torch.cumprod(torch.cat([torch.ones([N, 1], dtype=alpha.dtype), 1. - alpha + 1e-7], -1), -1)[:, :-1]
    weights_sum = weights.sum(dim=-1, keepdim=True)
    image = (color * weights[:, :, None]).sum(dim=1)
    ori_z = ((z - near[:, None]) / (far - near)[:, None]).clamp(0, 1)
    depth = torch.sum(weights * ori_z, dim=-1)
    image = image + (1 - weights_sum) * (1 if bg is None else bg)
    out = {"image": image, "weights_sum": weights_sum[:, 0], "depth": depth, "weights": weights}
    if normal is not None:
        out["normal_map"] = torch.sum(normal * weights[:, :, None], dim=1)
    return out


def composite_ref(z, sdf, normal, color, inv_s, rays_d, bg, near, far, num_steps, car, softplus=None):
    """models/instant_nsr.py:222-263, 290-294 -> image [N,3], weights_sum [N], depth [N], normal_map [N,3], weights [N,T], alpha [N,T]"""
    deltas = torch.cat([z[:, 1:] - z[:, :-1], ((far - near) / num_steps)[:, None]], dim=-1)
    true_cos = (rays_d[:, None, :] * normal).sum(-1)
    alpha = neus_alpha_ref(sdf, true_cos, deltas, inv_s, car, softplus)
    out = composite_from_alpha(alpha, color, z, near, far, bg, normal)
    out["alpha"] = alpha
    return out


def packed_shading_ref(sdf16, gradient, inv_s, xyzs, dirs, deltas, n_valid, car):
    """models/instant_nsr.py:215, 222-243, 266-272 on packed rows -> alpha [M], normal [M,3], eik [M,2] = (relax (|g| - 1)^2, relax)"""
    gn = torch.linalg.norm(gradient, ord=2, dim=-1, keepdim=True)
    normal = gradient / (1e-5 + gn)
    true_cos = (dirs * normal).sum(-1)
    dt = deltas if deltas.dim() == 1 else deltas[:, 0]
    alpha = neus_alpha_ref(sdf16[:, 0], true_cos, dt, inv_s.reshape(1), car)
    M = sdf16.shape[0]
    relax = ((torch.linalg.norm(xyzs, ord=2, dim=-1) < 1.2) & (torch.arange(M) < int(n_valid))).to(sdf16.dtype).detach()
    eik = torch.stack([relax * (gn[:, 0] - 1.0) ** 2, relax], dim=-1)
    return {"alpha": alpha, "normal": normal, "eik": eik}


def weight_norm_ref(v, g):
    """torch.nn.utils.weight_norm, dim 0: v [rows, cols], g [rows, 1]"""
    return torch._weight_norm(v, g, 0)


def variance_ref(variance):
    """SingleVarianceNetwork + forward_variance(): models/instant_nsr.py:35-45, 666-667"""
    return torch.exp(variance * 10.0).clip(1e-6, 1e6)


def variance_grad_ref(variance, g_inv_s_rows):
    """d / d variance of sum(rows * inv_s(variance)), by autograd through the clip"""
    v = variance.detach().clone().requires_grad_(True)
    (g_inv_s_rows * variance_ref(v)).sum().backward()
    return v.grad


def sds_upstream_ref(ws, gt, scale):
    """stylize.py:183-193 with reduction='sum': the opacity term of the stylisation loss"""
    return F.smooth_l1_loss(ws.clamp(0, 1), gt.clamp(0, 1), reduction="sum") * scale


def to_np(d):
    return {k: v.detach().double().numpy() for k, v in d.items() if v is not None}


# ---- composite -----------------------------------------------------------------------------------------------------------------------------------
SHORT_COUNTS = [(16, 16), (32, 64), (64, 128)]                    # composite_*_kernel<128, false>
LONG_COUNTS = [(17, 17), (36, 100), (100, 132), (256, 512)]       # composite_*_kernel<512, true>
INV_S = [20.0, 300.0, 3000.0]
CARS = [1.0, f32(0.3)]
RAY_COUNTS = [1, 3, 37]
MANY_RAYS = 4 * 4096 + 5                                          # the grid-stride loop's second trip (4096 workgroups of 4 rays)
LOSSES = {"all": ("image", "weights_sum", "depth", "normal_map"), "image": ("image",), "wsum_depth": ("weights_sum", "depth")}
COMPOSITE_OUTPUTS = ("image", "weights_sum", "depth", "normal_map", "weights", "alpha")
COMPOSITE_GRADS = ("g_sdf", "g_normal", "g_color", "g_inv_s")


def _comp_case(T0, T, inv_s, car, bg, N, loss="all", bound=1.6, grads=True, hit="mid"):
    return dict(T0=T0, T=T, inv_s=inv_s, car=car, bg=bg, N=N, loss=loss, bound=bound, grads=grads, hit=hit)


def composite_cases():
    cases = {}

    def add(c):
        cid = "T{T0}_{T}-s{inv_s:g}-c{car:.1f}-{b}-n{N}-{loss}-b{bound}".format(b="bg" if c["bg"] else "nobg", **c) + ("-last" if c["hit"] == "last" else "")
        assert cid not in cases
        cases[cid] = c
    for (T0, T), inv_s, car, bg in itertools.product(SHORT_COUNTS + LONG_COUNTS, INV_S, CARS, (True, False)):
        for N in RAY_COUNTS + ([MANY_RAYS] if T == 16 else []):
            add(_comp_case(T0, T, inv_s, car, bg, N))
    for (T0, T), loss, bound in itertools.product([(32, 64), (36, 100)], ("image", "wsum_depth"), (1.6, 1.0)):
        add(_comp_case(T0, T, 300.0, f32(0.3), True, 37, loss=loss, bound=bound))       # autograd hands None upstream gradients to the operator
    for (T0, T), inv_s, car in itertools.product([ct for ct in SHORT_COUNTS + LONG_COUNTS if ct[0] != ct[1]], (20.0, 300.0), CARS):
        add(_comp_case(T0, T, inv_s, car, True, 3, hit="last"))        # the last sample's delta = (far - near) / num_steps, num_steps != T, carries ray 0
    add(_comp_case(32, 64, 5e4, 1.0, True, 37, grads=False))                            # every gradient vanishes there: forward only
    return cases


def composite_inputs(c):
    """float32 CPU tensors of one case.  Ray 1 (where there is one) starts inside the cube; ray 2 has its first z before near and its last z past far."""
    N, T, T0, bound = c["N"], c["T"], c["T0"], c["bound"]
    key = ("composite", T0, T, c["inv_s"], c["car"], c["bg"], c["loss"], bound, c["hit"])
    tgt = _rs(*key, "tgt").uniform(-0.4, 0.4, (N, 3))
    o = _rs(*key, "o").normal(size=(N, 3))
    o = o / np.linalg.norm(o, axis=-1, keepdims=True) * _rs(*key, "r").uniform(2.4, 3.0, (N, 1))
    if N > 1:
        o[1] = 0.3 * tgt[1] + 0.1
    d = tgt - o
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    ro, rd = o.astype(F32), d.astype(F32)
    near, far = cube_near_far(ro, rd, bound)
    assert np.isfinite(near).all() and np.isfinite(far).all() and (far > near).all()
    if N > 1:
        assert near[1] == F32(0.05)
    n64, span = near.astype(np.float64)[:, None], (far.astype(np.float64) - near.astype(np.float64))[:, None]
    z = n64 + span * (np.arange(T)[None, :] + _rs(*key, "z").uniform(0.05, 0.95, (N, T))) / T
    if N > 2:
        z[2, 0], z[2, -1] = near[2] - 0.1, far[2] + 0.1
    z_hit = n64 + span * _rs(*key, "hit").uniform(0.3, 0.7, (N, 1))
    noise = 0.01 * _rs(*key, "noise").normal(size=(N, T))
    nrm = -d[:, None, :] + 0.3 * _rs(*key, "nrm").normal(size=(N, T, 3))
    nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    # ray 0: the far end of one sample's section lies on the surface (next_cdf = 1/2, where d alpha / d sdf is largest).  Sections are wide against
    # 1 / inv_s, so a ray with its crossing drawn anywhere usually has every sigmoid saturated and no gradient at all: with this ray no case is.
    # hit = "mid": the middle sample; "last": sample T - 1, whose delta is (far - near) / num_steps -- all of that ray's gradient goes through it.
    # ray 2: the same at its first (bg given) or last (no bg) sample, the ones outside [near, far]: a clamped depth term with weight.
    def pin(r, k):
        noise[r, :k] = np.abs(noise[r, :k])              # nothing crosses in front of the pinned sample: it has the ray's transmittance
        dk = z[r, k + 1] - z[r, k] if k < T - 1 else float(span[r, 0]) / T0
        tc = float((d[r] * nrm[r, k]).sum())
        ic = (np.logaddexp(0.0, 100.0 * (-tc * 0.5 + 0.5)) * (1.0 - c["car"]) + np.logaddexp(0.0, -100.0 * tc) * c["car"]) / 100.0
        z_hit[r] = z[r, k] + (ic * dk * 0.5 - noise[r, k]) / 0.6
    pin(0, T - 1 if c["hit"] == "last" else T // 2)
    if N > 2:
        pin(2, 0 if c["bg"] else T - 1)
    sdf = 0.6 * (z_hit - z) + noise
    inp = dict(rays_o=torch.from_numpy(ro), rays_d=torch.from_numpy(rd), near=torch.from_numpy(near), far=torch.from_numpy(far), z=_t(z), sdf=_t(sdf),
               normal=_t(nrm), color=_t(_rs(*key, "col").uniform(0, 1, (N, T, 3))), bg=_t(_rs(*key, "bg").uniform(0, 1, (N, 3))) if c["bg"] else None,
               inv_s=torch.tensor([[c["inv_s"]]], dtype=torch.float32))
    inp["up"] = {"image": _t(_rs(*key, "u_i").normal(size=(N, 3))), "weights_sum": _t(_rs(*key, "u_w").normal(size=N)),
                 "depth": _t(_rs(*key, "u_d").normal(size=N)), "normal_map": _t(_rs(*key, "u_n").normal(size=(N, 3)))}
    return inp


def weighted_loss(out, up, names):
    return sum((out[k] * up[k].to(out[k].dtype)).sum() for k in names)


def composite_eval(c, inp, dtype, per_ray_inv_s=False):
    """the restatement in dtype: outputs and, for a gradient case, gradients as float64 numpy arrays (per_ray_inv_s: g_inv_s per ray, [N])"""
    cv = lambda t: None if t is None else t.detach().clone().to(dtype)
    N = c["N"]
    sdf, nrm, col = (cv(inp[k]).requires_grad_(c["grads"]) for k in ("sdf", "normal", "color"))
    inv_s = (cv(inp["inv_s"]).expand(N, 1).clone() if per_ray_inv_s else cv(inp["inv_s"])).requires_grad_(c["grads"])
    out = composite_ref(cv(inp["z"]), sdf, nrm, col, inv_s, cv(inp["rays_d"]), cv(inp["bg"]), cv(inp["near"]), cv(inp["far"]), c["T0"], c["car"])
    res = dict(out)
    if c["grads"]:
        weighted_loss(out, inp["up"], LOSSES[c["loss"]]).backward()
        res.update(g_sdf=sdf.grad, g_normal=nrm.grad, g_color=col.grad if col.grad is not None else torch.zeros_like(col), g_inv_s=inv_s.grad.reshape(-1))
    return to_np(res)


# ---- packed_shading ------------------------------------------------------------------------------------------------------------------------------
PACKED_M = [1, 255, 257, 1000]
PACKED_OUTPUTS = ("alpha", "normal", "eik")
PACKED_GRADS = ("g_sdf16", "g_gradient", "g_gradient_zero_rows", "g_inv_s")    # the rows with gradient == 0 carry d normal / d g = I / 1e-5: a tensor of their own


def packed_cases():
    cases = {}

    def add(M, nv, stride, inv_s, car, drop=None):
        cid = f"M{M}-v{nv}-d{stride}-s{inv_s:g}-c{car:.1f}" + (f"-no_{drop}" if drop else "")
        cases[cid] = dict(M=M, n_valid=nv, stride=stride, inv_s=inv_s, car=car, drop=drop)
    for M, stride, inv_s, car in itertools.product(PACKED_M, (1, 2), INV_S, CARS):
        for nv in sorted({M, max(M - 7, 0), 0}):
            add(M, nv, stride, inv_s, car)
    for drop, stride in itertools.product(PACKED_OUTPUTS, (1, 2)):                 # each upstream gradient None in turn
        add(257, 250, stride, 300.0, f32(0.3), drop)
    return cases


def packed_zero_rows(M):
    return sorted({0, M // 2, M - 1}) if M >= 3 else []


def packed_inputs(c):
    M, key = c["M"], ("packed", c["stride"], c["inv_s"], c["car"], c["drop"])
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    g = unit(_rs(*key, "g").normal(size=(M, 3))) * _rs(*key, "gn").uniform(0.2, 3.0, (M, 1))
    g[packed_zero_rows(M)] = 0.0
    x = unit(_rs(*key, "x").normal(size=(M, 3))) * _rs(*key, "xn").uniform(0.8, 1.6, (M, 1))
    if M >= 8:                                             # one row on each side of |x| = 1.2, within 1e-6
        x[3], x[4] = unit(x[3]) * (1.2 - 8e-7), unit(x[4]) * (1.2 + 8e-7)
    x = x.astype(F32)
    n32 = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    assert ((n32 < F32(1.2)) == (np.linalg.norm(x.astype(np.float64), axis=-1) < 1.2)).all()       # both precisions see every row on the same side
    if M >= 8:
        assert n32[3] < F32(1.2) <= n32[4] and abs(float(n32[3]) - 1.2) < 1e-6 and abs(float(n32[4]) - 1.2) < 1e-6
    sdf16 = _rs(*key, "s16").normal(size=(M, 16))
    sdf16[:, 0] = _rs(*key, "sdf").uniform(-3.0, 3.0, M) / c["inv_s"]              # a few widths of the sigmoid around the surface
    deltas = _rs(*key, "dt").uniform(0.002, 0.03, (M, 2) if c["stride"] == 2 else M)
    dirs = unit(_rs(*key, "d").normal(size=(M, 3)))
    # one row faces the ray with the far end of its section on the surface (next_cdf = 1/2, d alpha / d sdf = -inv_s / 4): no case without a gradient
    r = 0 if M < 3 else 1
    dirs[r], sdf16[r, 0] = -unit(g[r]), 0.5 * float(np.reshape(deltas, (M, -1))[r, 0])
    inp = dict(sdf16=_t(sdf16), gradient=_t(g), xyzs=torch.from_numpy(x), dirs=_t(dirs), deltas=_t(deltas),
               inv_s=torch.tensor([[c["inv_s"]]], dtype=torch.float32))
    inp["up"] = {"alpha": _t(_rs(*key, "u_a").normal(size=M)), "normal": _t(_rs(*key, "u_n").normal(size=(M, 3))), "eik": _t(_rs(*key, "u_e").normal(size=(M, 2)))}
    return inp


def packed_loss_names(c):
    return tuple(k for k in PACKED_OUTPUTS if k != c["drop"])


def packed_split(c, g_gradient):
    """-> (rows with |g| > 0, the rows with gradient == 0) of a [M,3] array"""
    zr = packed_zero_rows(c["M"])
    keep = np.setdiff1d(np.arange(c["M"]), zr)
    return g_gradient[keep], g_gradient[zr]


def packed_eval(c, inp, dtype):
    cv = lambda t: t.detach().clone().to(dtype)
    sdf16, g, inv_s = (cv(inp[k]).requires_grad_(True) for k in ("sdf16", "gradient", "inv_s"))
    out = packed_shading_ref(sdf16, g, inv_s, cv(inp["xyzs"]), cv(inp["dirs"]), cv(inp["deltas"]), c["n_valid"], c["car"])
    weighted_loss(out, inp["up"], packed_loss_names(c)).backward()
    res = to_np(out)
    gg = g.grad.double().numpy()
    res["g_gradient"], res["g_gradient_zero_rows"] = packed_split(c, gg)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)                # no alpha in the loss: nothing reaches sdf16 and inv_s
    res["g_sdf16"], res["g_inv_s"] = zero(sdf16).double().numpy(), zero(inv_s).double().numpy().reshape(-1)
    return res


# ---- weight norm and its backward, the bias and variance gradients ----------------------------------------------------------------------------------
WN_SHAPES = [(1, 1), (64, 3), (65, 37), (16, 64), (3, 300), (5, 257)]
WN_MAX_LAYERS, PG_MAX_ENTRIES = 8, 12                      # AC_WN_MAX_LAYERS, AC_PG_MAX_ENTRIES
WN_PAD = 3                                                 # row-strided views: stride = cols + WN_PAD
ADD_CASES = [(rows, stride) for rows in (1, 16, 300) for stride in (1, 36)]
VARIANCE_ROWS = [1, 255, 4096, 5000]
VARIANCE_INSIDE = [f32(0.3), f32(0.6), f32(-0.9)]          # inv_s = 20, 403, 1.2e-4
VARIANCE_CLIPPED = [f32(-1.5), f32(1.5)]                   # exp(10 v) = 3e-7 < 1e-6 and 3e6 > 1e6


def wn_layer(rows, cols, tag=0):
    """v, g, an upstream d W and old contents of the two destinations"""
    key = ("wn", rows, cols, tag)
    return dict(v=_t(_rs(*key, "v").normal(size=(rows, cols))), g=_t(_rs(*key, "g").uniform(0.5, 2.0, (rows, 1)) * _rs(*key, "sg").choice([-1.0, 1.0], (rows, 1))),
                gw=_t(_rs(*key, "gw").normal(size=(rows, cols))), old_v=_t(_rs(*key, "ov").normal(size=(rows, cols))), old_g=_t(_rs(*key, "og").normal(size=(rows, 1))))


def wn_eval(layer, dtype):
    v, g = (layer[k].detach().clone().to(dtype).requires_grad_(True) for k in ("v", "g"))
    w = weight_norm_ref(v, g)
    (w * layer["gw"].to(dtype)).sum().backward()
    return to_np(dict(w=w, g_v=v.grad, g_g=g.grad))


def wn_cases():
    """layer id -> (rows, cols, tag): every shape alone, and the 8 layers of the full launch (tags 1..8, mixed shapes)"""
    cases = {f"r{r}c{c}": (r, c, 0) for r, c in WN_SHAPES}
    for i in range(WN_MAX_LAYERS):
        r, c = WN_SHAPES[(5 * i + 2) % len(WN_SHAPES)]
        cases[f"full{i}-r{r}c{c}"] = (r, c, i + 1)
    return cases


def add_inputs(rows, stride):
    key = ("add", rows, stride)
    return dict(src=_t(_rs(*key, "src").normal(size=(rows, stride))), old=_t(_rs(*key, "old").normal(size=rows)))


def variance_cases():
    return {f"v{v:g}-n{n}": dict(variance=v, rows=n) for v in VARIANCE_INSIDE + VARIANCE_CLIPPED for n in VARIANCE_ROWS}


def variance_inputs(c):
    """per-ray partials of d loss / d inv_s with a mean away from zero, so that their sum's condition number stays bounded"""
    return dict(variance=torch.tensor(c["variance"], dtype=torch.float32), rows=_t(_rs("var", c["rows"]).normal(0.3, 1.0, c["rows"])),
                old=_t(_rs("var", c["rows"], "old").normal(size=1)))


def variance_eval(c, inp, dtype):
    return {"g_variance": variance_grad_ref(inp["variance"].to(dtype), inp["rows"].to(dtype)).double().numpy().reshape(1)}


# ---- sds_upstream --------------------------------------------------------------------------------------------------------------------------------
SDS_N = [1, 1023, 1024, 1025, 4096, 65536]
SDS_EDGE = [-0.1, 0.0, 1.0, 1.1, 0.5]


def sds_cases():
    cases = {f"n{n}": dict(N=n, pairs=False) for n in SDS_N}
    cases["pairs"] = dict(N=len(SDS_EDGE) ** 2, pairs=True)        # every (weights_sum, weights_sum_gt) from SDS_EDGE x SDS_EDGE
    return cases


def sds_inputs(c):
    N = c["N"]
    if c["pairs"]:
        ws, gt = (np.array(a, np.float64) for a in zip(*itertools.product(SDS_EDGE, SDS_EDGE)))
    else:
        ws, gt = _rs("sds", "ws").uniform(-0.2, 1.2, N), _rs("sds", "gt").uniform(-0.2, 1.2, N)
        ws[0], gt[0] = 0.3, 0.8                                    # the one ray of N = 1 lies inside [0, 1]: a gradient to check
    return dict(ws=_t(ws), gt=_t(gt), scale=f32(1e5 / N))


def sds_eval(c, inp, dtype):
    ws = inp["ws"].detach().clone().to(dtype).requires_grad_(True)
    loss = sds_upstream_ref(ws, inp["gt"].to(dtype), inp["scale"])
    loss.backward()
    return to_np(dict(loss=loss.reshape(1), g_ws=ws.grad))


# ---- everything the bounds file records -------------------------------------------------------------------------------------------------------------
# the gradient tensors whose largest float64 entry must reach GMAX_MIN (a 1 x 1 weight-norm layer has d v == 0: w = sign(v) g)
GMAX_KEY = {"composite": ("g_sdf",), "packed_shading": ("g_gradient",), "weight_norm": ("g_v", "g_g"), "variance": (), "sds_upstream": ("g_ws",)}


def families():
    """family -> (cases, evaluate(case, dtype) -> {tensor: float64 array}, is a gradient case)"""
    return {
        "composite": (composite_cases(), lambda c, dt: composite_eval(c, composite_inputs(c), dt), lambda c: c["grads"]),
        "packed_shading": (packed_cases(), lambda c, dt: packed_eval(c, packed_inputs(c), dt), lambda c: True),
        "weight_norm": (wn_cases(), lambda c, dt: wn_eval(wn_layer(*c), dt), lambda c: True),
        "variance": (variance_cases(), lambda c, dt: variance_eval(c, variance_inputs(c), dt), lambda c: False),
        "sds_upstream": (sds_cases(), lambda c, dt: sds_eval(c, sds_inputs(c), dt), lambda c: True),
    }


def measure(r32, r64):
    """{tensor: [err32, max|f64|]} of one case evaluated in both precisions"""
    rec = {}
    for k in sorted(r64):
        a, b = r32[k], r64[k]
        assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all(), k
        rec[k] = [float(np.abs(a - b).max()) if b.size else 0.0, float(np.abs(b).max()) if b.size else 0.0]
    return rec
