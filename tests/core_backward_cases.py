"""Cases and the restatement for the whole training backward, nsr_ops.render_core_backward (csrc/render_core_backward.hip: core_normals_kernel ->
compositor -> colour network -> core_mid_kernel -> SDF query, with or without saved stencil features -> table scatter), compared FROM ITS SAVED STATE
with float64 autograd.  GPU tier: tests/test_gpu_core_backward.py, CPU tier: tests/test_core_backward_host.py, bounds of family A:
tests/golden/make_core_backward_bounds.py -> tests/golden/core_backward_bounds.json.  The rule and its constants are those of tests/step_op_cases.py.

Plain torch on the CPU, no GPU import.  The backward works from plain tensors -- z_vals, pts, sdf, sdf_out16, gradient, color, eik_den (and feat7) -- and
nothing makes them agree with each other, so the restatement is the chain of vector-Jacobian products AT THE SAVED VALUES: the reference's own lines,
composed from tests/field_op_cases.py and tests/step_op_cases.py, in which every saved quantity enters by value substitution,
v = saved + (chain - chain.detach()):
  1. sdf_query_ref at pts -> out16, gradient; 2. the saved sdf_out16 and gradient take their place, sdf is the saved sdf with its gradient routed to
  out16[:, 0]; 3. normal = g / (1e-5 + |g|) (models/instant_nsr.py:215); 4. color_ref(pts, normal, out16), then the saved color; 5. composite_ref with the
  saved z_vals; 6. loss = upstream-weighted sum of image, weights_sum, depth, normal_map + sum over eikonal groups of g_eik relax (|g| - 1)^2 / eik_den,
  relax = |p| < 1.2 and eik_den constants (:266-272).
Modes: float32, float64 and K, the declared arithmetic of tests/field_op_cases.py (table softplus -- also where the compositor forms iter_cos from
true_cos: composite.hip evaluates the same cubic and, backwards, its derivative -- bf16 splits, record rounding; everything else float32).  K of the saved-feature variant (sdf_stencil_bwd_kernel<SAVED = true>) forms dW1 += d1 inp^T as that kernel's header declares it: both
factors split hi + lo, each part rounded to nearest, hi hi + lo hi + hi lo, float32 sums; db1 is the column of ones of the same product.

Family A draws every saved tensor (feat7 = None: the re-gathering backward); its bounds are recorded on the CPU.  Candidate RAYS are rejected, not
samples: a ray fails if one of its samples fails color_rows_pass, has |true_cos| < 2^-12 |d| |g| or has ||p| - 1.2| < 2^-12 (the samples placed on
purpose aside: the one with gradient == 0 has true_cos == 0 in every precision, the two next to |p| = 1.2 are asserted to lie on the same side in both).
4 N candidates, the first N that pass.
Family B takes the state of a training forward on the golden field (the GPU tier reads it back, the CPU tier estimates from the oracle's forward how
many rays its rule leaves): see family_b_keep."""
import numpy as np
import torch

from tests import field_op_cases as FC
from tests import step_op_cases as SC
from tests.field_op_cases import (stencil_points, geometry, encode, sdf_query_ref, sdf_query_declared, color_ref, declared_table_gradient, table_of,   # noqa: F401
                                  weights_of, sdf_points, color_rows_pass)
from tests.step_op_cases import composite_ref, neus_alpha_ref, FACTOR, FLOOR, GMAX_MIN, _rs, _t          # noqa: F401

F32, K, BOUND, EPS, LEVELS = FC.F32, FC.K, FC.BOUND, FC.EPS, FC.LEVELS
K_SAVED = "K_saved"                                        # K with the saved-feature variant's dW1
COS_MARGIN_A, RELAX_MARGIN = 2.0 ** -12, 2.0 ** -12
GATE_MARGIN_B, COS_MARGIN_B = 2.0 ** -16, 2.0 ** -20       # family B: four times float32's worst rounding of a 64-term dot product
LEGACY = 3e-4                                              # an "open" tensor: the tolerance the suite applied before, of max|f64|
WEIGHT_TENSORS = tuple("g_" + k for k in FC.SDF_W + FC.COLOR_W)
TENSORS = WEIGHT_TENSORS + ("g_inv_s",) + FC.TABLE_TENSORS
UPSTREAMS = {"all": ("image", "weights_sum", "depth", "normal_map", "eik"), "image": ("image",), "normal_map": ("normal_map",), "eikonal": ("eik",)}
MUTANTS = ("no_relax", "k_with_c", "no_comp_normal", "sdf_all_columns", "one_den", "recomputed_gradient", "dw1_hi_only")


def bound_of(err32, errK, max64, factor=FACTOR):
    return factor * max(err32, errK) + FLOOR * max64


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------
def geometry_f32(x32, scale_mode):
    """FC.geometry with the cells a float32 evaluation chooses for itself: the stencil points and u * scale + 0.5 formed in float32 (f32_mul_add:
    torch's two roundings, f32_fma: the kernels' one)"""
    pts = stencil_points(torch.from_numpy(np.ascontiguousarray(x32, F32))).numpy()
    cell = np.floor(FC.cell_positions(pts, scale_mode)).astype(np.int64)
    glob = FC.corner_rows(cell)
    rows, slot = np.unique(glob, return_inverse=True)
    return dict(cell=torch.from_numpy(cell), rows=rows, slot=torch.from_numpy(slot.reshape(glob.shape)), seg=np.searchsorted(rows, FC.table_offsets()))


def _subst(saved, chain):
    return saved + (chain - chain.detach())


def core_eval(st, mode, mutant=None, own_cells=False):
    """the chain at the saved values of the state st (float32 CPU tensors, see draw_state) -> {tensor: float64 array} and "rows": the table rows the
    table gradients refer to (g_table_Lxx: [rows of that level, 2], in the order of rows).  mode: torch.float32 / torch.float64 / K / K_SAVED.
    own_cells (family B): a float32 evaluation takes the cells of its own float32 positions (float32: torch's, K: the kernels' fma)"""
    declared = mode in (K, K_SAVED)
    dt = torch.float32 if declared else mode
    N, T = st["z"].shape
    B = N * T
    cv = lambda t: None if t is None else t.detach().clone().to(dt)
    x32 = st["pts"].reshape(B, 3)
    if own_cells and dt == torch.float32:
        geo = geometry_f32(x32.numpy(), "f32_fma" if declared else "f32_mul_add")
    else:
        geo = st.get("geo") or geometry(x32.numpy())
    Wt = weights_of(st["weights"])
    Ws = [Wt[k].detach().clone().to(dt).requires_grad_(True) for k in FC.SDF_W]
    Wc = [Wt[k].detach().clone().to(dt).requires_grad_(True) for k in FC.COLOR_W]
    leaf = torch.from_numpy(table_of(st["weights"])[geo["rows"]]).to(dt).requires_grad_(not declared)
    x = cv(x32)
    p7 = stencil_points(x)
    feat, w = encode(p7, geo, leaf)
    if declared:
        feat_d = feat.detach().requires_grad_(True)
        dw1 = None if mode == K else ("hi" if mutant == "dw1_hi_only" else "split")
        out16_c, grad_c = sdf_query_declared(p7.detach(), feat_d, *Ws, dw1=dw1)
    else:
        out16_c, grad_c = sdf_query_ref(p7, feat, *Ws)
    out16 = _subst(cv(st["out16"]).reshape(B, 16), out16_c)
    g = _subst(cv(st["gradient"]).reshape(B, 3), grad_c)
    d_sdf = out16_c if mutant == "sdf_all_columns" else out16_c[:, :1]     # (mutant: d sdf lands in every column of d sdf_out16)
    sdf = cv(st["sdf"]).reshape(B) + (d_sdf - d_sdf.detach()).sum(-1)
    r = torch.linalg.norm(g, ord=2, dim=-1, keepdim=True)
    c = 1e-5 + r
    normal = g / c                                                         # models/instant_nsr.py:215
    if mutant == "k_with_c":                                               # d (1 / c) / d g = -g / (r c) instead of -g / (r c^2)
        normal = g / c.detach() + g.detach() * (-(r - r.detach()) / c.detach())
    n_col = normal
    if mutant == "recomputed_gradient":                                    # the colour network sees the query's own gradient, not the saved one
        gc = grad_c.detach() + (g - g.detach())
        n_col = gc / (1e-5 + torch.linalg.norm(gc, ord=2, dim=-1, keepdim=True))
    col_c = color_ref(x, n_col, out16, *Wc, declared=declared)
    color = _subst(cv(st["color"]).reshape(B, 3), col_c)
    inv_s = cv(st["inv_s"]).reshape(1, 1).expand(N, 1).clone().requires_grad_(True)
    n_comp = normal.detach() if mutant == "no_comp_normal" else normal
    out = composite_ref(cv(st["z"]), sdf.reshape(N, T), n_comp.reshape(N, T, 3), color.reshape(N, T, 3), inv_s, cv(st["rays_d"]), cv(st["bg"]),
                        cv(st["near"]), cv(st["far"]), st["T0"], st["car"], softplus=FC.TableSoftplus.apply if declared else None)
    up = st["up"]
    loss = sum((out[k] * up[k].to(dt)).sum() for k in ("image", "weights_sum", "depth", "normal_map") if up.get(k) is not None)
    if up.get("eik") is not None:
        relax = (torch.linalg.norm(cv(st["pts"]).reshape(B, 3), ord=2, dim=-1) < 1.2).to(dt)
        if mutant == "no_relax":
            relax = torch.ones_like(relax)
        G = up["eik"].numel()
        den = cv(st["eik_den"]).reshape(G)
        if mutant == "one_den":
            den = den[:1].expand(G)
        grp = torch.arange(B) // (st["group_rays"] * T) if st["group_rays"] else torch.zeros(B, dtype=torch.long)
        loss = loss + (up["eik"].to(dt)[grp] * relax * (r[:, 0] - 1.0) ** 2 / den[grp]).sum()
    loss = loss + 0.0 * sum(t.sum() for t in Ws + Wc) + 0.0 * inv_s.sum() + (0.0 * leaf.sum() if not declared else 0.0 * feat_d.sum())
    loss.backward()
    g_rows = declared_table_gradient(w, feat_d.grad, geo) if declared else FC._np64(leaf.grad)
    res = {"g_" + k: FC._np64(t.grad) for k, t in zip(FC.SDF_W + FC.COLOR_W, Ws + Wc)}
    res["g_inv_s"] = FC._np64(inv_s.grad).reshape(N)
    res.update(FC._per_level(g_rows, geo))
    res["rows"] = geo["rows"]
    return res


def on_rows(res, rows):
    """the result's table gradients on the given (sorted) rows of the whole table, zeros where it touched none: {tensor: array} without "rows" """
    own = np.concatenate([res[k] for k in FC.TABLE_TENSORS])
    full = np.zeros((len(rows), 2))
    at = np.searchsorted(rows, res["rows"])
    assert np.array_equal(rows[at], res["rows"])
    full[at] = own
    seg = np.searchsorted(rows, FC.table_offsets())
    out = {k: v for k, v in res.items() if k != "rows" and k not in FC.TABLE_TENSORS}
    out.update({name: full[seg[l]:seg[l + 1]] for l, name in enumerate(FC.TABLE_TENSORS)})
    return out


def union_rows(*row_sets):
    return np.unique(np.concatenate([np.asarray(r, np.int64) for r in row_sets]))


def measure(r32, rK, r64, extra_rows=()):
    """-> (rows, float64 result on them, {tensor: [err32, errK, max|f64|]}): the three modes on the union of the rows any of them (or extra_rows) touched"""
    rows = union_rows(r32["rows"], rK["rows"], r64["rows"], extra_rows)
    a, b, ref = (on_rows(r, rows) for r in (r32, rK, r64))
    return rows, ref, FC.measure3(a, b, ref)


# ---- family A: drawn state -----------------------------------------------------------------------------------------------------------------------------
def case_a(N, T0, up, inv_s=300.0, car=1.0, weights="golden", loss="all", group_rays=0, edges=False):
    return dict(N=N, T0=T0, up=up, inv_s=inv_s, car=car, weights=weights, loss=loss, group_rays=group_rays, edges=edges)


def cases_a():
    cases = {}

    def add(c):
        cid = "n{N}-T{T0}_{up}-s{inv_s:g}-c{car:.1f}-{weights}-{loss}".format(**c) + (f"-grp{c['group_rays']}" if c["group_rays"] else "")
        assert cid not in cases and c["N"] * (c["T0"] + c["up"]) < 2000
        cases[cid] = c
    car3 = SC.f32(0.3)
    add(case_a(1, 16, 16))
    add(case_a(5, 16, 16, 20.0, car3))
    add(case_a(37, 16, 16, edges=True))
    add(case_a(37, 16, 16, 300.0, car3, "drawn", edges=True))
    add(case_a(1, 32, 32, 20.0, car3, "drawn"))
    add(case_a(5, 32, 32))
    add(case_a(5, 32, 32, 20.0, 1.0, "drawn", edges=True))
    add(case_a(1, 40, 16, 300.0, car3))                    # the long compositor; T = 56: a 16-row tile straddles two rays
    add(case_a(5, 40, 16, edges=True))
    add(case_a(5, 40, 16, 20.0, car3, "drawn"))
    add(case_a(37, 2, 16))
    add(case_a(5, 2, 16, 20.0, car3, "drawn"))
    for loss in ("image", "normal_map", "eikonal"):
        add(case_a(37, 16, 16, loss=loss, edges=True))
        add(case_a(5, 40, 16, 300.0, car3, "drawn", loss=loss))
    add(case_a(5, 16, 16, group_rays=3))                   # two eikonal groups: rays 0..2 and 3..4
    add(case_a(5, 40, 16, 20.0, car3, "drawn", group_rays=3))
    return cases


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _norm32(p):
    """|p| as core_mid_kernel forms it"""
    p = np.ascontiguousarray(p, F32)
    return np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])


def ray_rules(pts, gradient, out16, rays_d, Wt, exempt_cos=None, exempt_relax=None, gate_margin=FC.GATE_MARGIN, cos_margin=COS_MARGIN_A,
              relax_margin=RELAX_MARGIN):
    """float32 arrays [M,T,..] -> bool [M]: the ray passes (no sample fails a rule); exempt_*: bool [M,T] of samples a rule does not apply to"""
    M, T = pts.shape[:2]
    p, g, o, d = (np.asarray(a, F32).astype(np.float64) for a in (pts, gradient, out16, rays_d))
    gn = np.linalg.norm(g, axis=-1, keepdims=True)
    n = g / (1e-5 + gn)
    gates = ~color_rows_pass(p.reshape(-1, 3), n.reshape(-1, 3), o.reshape(-1, 16), Wt, margin=gate_margin).reshape(M, T)
    cos = np.abs((d[:, None, :] * g).sum(-1)) < cos_margin * np.linalg.norm(d, axis=-1)[:, None] * gn[..., 0]
    cos |= gn[..., 0] == 0.0
    if exempt_cos is not None:
        cos &= ~exempt_cos
    relax = np.abs(np.linalg.norm(p, axis=-1) - 1.2) < relax_margin
    if exempt_relax is not None:
        relax &= ~exempt_relax
    return ~(gates | cos | relax).any(-1)


OUT16_TRIES = 8


def draw_out16(key, pts, gradient, Wt):
    """sdf_out16 [M,T,16] as color_inputs draws it.  One sample in 13 has one of its 128 hidden units within GATE_MARGIN, so hardly a whole ray of 32 or
    64 independent draws would pass color_rows_pass: each SAMPLE takes the first of OUT16_TRIES draws of its own row that passes (with its position and
    normal as they are), and the ray rule then still rejects a ray with a sample for which none did"""
    M, T = pts.shape[:2]
    cand = _rs(*key, "o").normal(0.0, 0.3, (M, T, OUT16_TRIES, 16)).astype(F32)
    g = gradient.astype(np.float64)
    n = (g / (1e-5 + np.linalg.norm(g, axis=-1, keepdims=True))).astype(F32).astype(np.float64)
    rep = lambda a: np.repeat(a.astype(np.float64).reshape(M * T, 1, 3), OUT16_TRIES, 1).reshape(-1, 3)
    ok = color_rows_pass(rep(pts), rep(n), cand.astype(np.float64).reshape(-1, 16), Wt).reshape(M, T, OUT16_TRIES)
    first = np.where(ok.any(-1), ok.argmax(-1), 0)
    return np.take_along_axis(cand, first[:, :, None, None], 2)[:, :, 0]


ZERO_RAY_SCALE = 2.0 ** -17


def _zero_gradient_sample(comp, gradient, ray, T0, car):
    """the sample of the ray that gets gradient == 0: its heaviest one (with that gradient zeroed), where the compositing weight is well conditioned.
    There d normal / d g = I / 1e-5, so the ray's per-ray upstreams are scaled by ZERO_RAY_SCALE (draw_state): 1e5 times that brings the sample to the
    level of the other rays' -- neither nothing nor everything.  (A sample that is light by itself will not do: behind the surface its weight is a
    product of factors 1 - alpha + 1e-7 with alpha within 1e-5 of 1, which keep two digits in float32, and in front of it a weight of 1e-6 is the
    1e-5 of alpha's numerator, where d alpha is the cancellation pc - nc.)"""
    one = lambda k: comp[k][ray:ray + 1].double()
    g0 = torch.from_numpy(gradient[ray:ray + 1].astype(np.float64))
    best, at = -1.0, 0
    for j in range(gradient.shape[1]):
        g = g0.clone()
        g[0, j] = 0.0
        n = g / (1e-5 + torch.linalg.norm(g, ord=2, dim=-1, keepdim=True))
        w = float(composite_ref(one("z"), one("sdf"), n, one("color"), comp["inv_s"].double(), one("rays_d"), one("bg"), one("near"), one("far"), T0, car)["weights"][0, j])
        if w > best:
            best, at = w, j
    return at


def draw_state(c):
    """float32 CPU tensors of one family-A case (+ "where": the samples placed on purpose, as (ray, sample) of the kept rays, and "passed": how many of
    the 4 N candidate rays pass)"""
    N, T0, T = c["N"], c["T0"], c["T0"] + c["up"]
    M = 4 * N
    key = ("core", T0, T, c["inv_s"], c["car"], c["weights"], c["loss"], c["group_rays"], c["edges"])
    Wt = weights_of(c["weights"])
    comp = SC.composite_inputs(SC._comp_case(T0, T, c["inv_s"], c["car"], True, M))      # z with a surface crossing mid-ray, rays, colour, upstreams
    x, where_x = sdf_points(key, M * T)
    pts = x.reshape(M, T, 3).copy()
    length = _rs(*key, "gl").uniform(0.1, 2.0, (M, T, 1))
    gradient = (comp["normal"].double().numpy() * length).astype(F32)
    ex_cos, ex_relax, where = np.zeros((M, T), bool), np.zeros((M, T), bool), {}
    rays_d = comp["rays_d"].numpy()
    out16 = draw_out16(key, pts, gradient, Wt)
    ok = ray_rules(pts, gradient, out16, rays_d, Wt)
    if c["edges"]:
        assert N >= 5
        edge_ray, zero_ray = (int(v) for v in np.flatnonzero(ok)[1:3])      # two rays that pass as drawn carry the samples placed on purpose
        taken, placed = {row % T for row in where_x.values() if row // T == edge_ray}, []
        for j in range(T):                                 # |p| on each side of 1.2, within 1e-6, on samples whose stencil stays clear of the cell faces
            if len(placed) == 2:
                break
            q = (_unit(pts[edge_ray, j].astype(np.float64)) * (1.2 + (-8e-7 if not placed else 8e-7))).astype(F32)
            n32, inside = float(_norm32(q)), not placed
            if (j not in taken and FC.sdf_rows_pass(q[None])[0] and (n32 < F32(1.2)) == inside == (np.linalg.norm(q.astype(np.float64)) < 1.2)
                    and abs(n32 - 1.2) < 1e-6):
                pts[edge_ray, j] = q
                ex_relax[edge_ray, j] = True
                placed.append(j)
        assert len(placed) == 2
        where.update(inside=(edge_ray, placed[0]), outside=(edge_ray, placed[1]))
        jz = _zero_gradient_sample(comp, gradient, zero_ray, T0, c["car"])
        gradient[zero_ray, jz] = 0.0
        ex_cos[zero_ray, jz] = True
        where["zero_gradient"] = (zero_ray, jz)
        row = where_x["near_plus_bound"]                   # sdf_points' own edge row: x_2 + eps is clamped at +bound
        where["clamped"] = (row // T, row % T)
        out16 = draw_out16(key, pts, gradient, Wt)         # (a sample's row depends on its own position and normal alone: the other samples keep theirs)
        ok = ray_rules(pts, gradient, out16, rays_d, Wt, ex_cos, ex_relax)
    keep = np.flatnonzero(ok)[:N]
    assert len(keep) == N, (c, int(ok.sum()))
    for name, (ray, j) in list(where.items()):
        assert ray in keep, (c, name, "the ray with the edge sample was rejected")
        where[name] = (int(np.searchsorted(keep, ray)), j)
    G = (N + c["group_rays"] - 1) // c["group_rays"] if c["group_rays"] else 1
    per = c["group_rays"] * T if c["group_rays"] else N * T
    relax = (np.linalg.norm(pts[keep].astype(np.float64), axis=-1) < 1.2).reshape(-1)
    den = np.array([relax[k * per:(k + 1) * per].sum() + 1e-5 for k in range(G)])                 # models/instant_nsr.py:266-272
    tk = lambda a: torch.from_numpy(np.ascontiguousarray(a[keep]))
    names = UPSTREAMS[c["loss"]]
    up = {k: (comp["up"][k][keep].clone() if k in names else None) for k in ("image", "weights_sum", "depth", "normal_map")}
    if c["edges"]:
        for v in up.values():
            if v is not None:
                v[where["zero_gradient"][0]] *= ZERO_RAY_SCALE
    up["eik"] = _t(_rs(*key, "u_e").uniform(0.5, 2.0, G) * _rs(*key, "u_es").choice([-1.0, 1.0], G)) if "eik" in names else None
    pick = lambda k: comp[k][keep].contiguous()
    return dict(N=N, T0=T0, T=T, car=c["car"], weights=c["weights"], group_rays=c["group_rays"], inv_s=comp["inv_s"], rays_o=pick("rays_o"),
                rays_d=pick("rays_d"), near=pick("near"), far=pick("far"), bg=pick("bg"), z=pick("z"), sdf=pick("sdf"), color=pick("color"), pts=tk(pts),
                gradient=tk(gradient), out16=tk(out16), eik_den=_t(den), up=up, where=where, passed=int(ok.sum()))


def eval_a(c, modes, mutant=None):
    st = draw_state(c)
    st["geo"] = geometry(st["pts"].reshape(-1, 3).numpy())
    return [core_eval(st, m, mutant) for m in modes]


# ---- family B: the forward's own state -----------------------------------------------------------------------------------------------------------------
CASES_B = {"T16_16": dict(T0=16, up=16, rays=(4, 6), long=False), "T32_32": dict(T0=32, up=32, rays=(3, 4), long=False),
           "long-T40_16": dict(T0=40, up=16, rays=(4, 6), long=True)}
B_INV_S, B_CAR, B_MAX_ZEROED, B_MAX_ESTIMATE = None, 1.0, 0.5, 0.25       # inv_s: the golden field's


# make_rays' default view (yaw 0.35, pitch -0.2) loses 6 of 24, 2 of 12 and 10 of 24 rays to the rule (one sample in ~150 has a hidden unit within the
# margin: a ray of 56 samples passes with probability ~0.7); this pitch 3 of 24, 2 of 12 and 6 of 24
B_VIEW = dict(yaw=0.35, pitch=0.1)


def rays_b(c):
    from tests.common import make_rays
    h, w = c["rays"]
    return make_rays(h, w, dist=1.7, f=6.4 * w / 4, **B_VIEW)


def inputs_b(c):
    """rays, fixed noise, background and upstream draws of one family-B case (float32 arrays)"""
    ro, rd = rays_b(c)
    N, key = ro.shape[0], ("coreB", c["T0"], c["up"])
    f = lambda a: np.ascontiguousarray(a, F32)
    up = {"image": f(_rs(*key, "u_i").normal(size=(N, 3))), "weights_sum": f(_rs(*key, "u_w").normal(size=N)), "depth": f(_rs(*key, "u_d").normal(size=N)),
          "normal_map": f(_rs(*key, "u_n").normal(size=(N, 3))), "eik": f([0.7])}
    return dict(rays_o=ro, rays_d=rd, noise=f(_rs(*key, "noise").uniform(0, 1, (N, c["T0"]))), bg=f(_rs(*key, "bg").uniform(0, 1, (N, 3))), up=up)


def family_b_keep(pts, gradient, out16, rays_d, weights="golden"):
    """the rule of family B on the float32 state: bool [N], False = the ray is zeroed in every per-ray upstream (it stays in the launch)"""
    return ray_rules(pts, gradient, out16, rays_d, weights_of(weights), gate_margin=GATE_MARGIN_B, cos_margin=COS_MARGIN_B, relax_margin=0.0)


def state_b(c, inp, saved, inv_s, keep):
    """the state core_eval takes, from the arrays a forward produced (saved: z_vals, pts, sdf, sdf_out16, gradient, color, eik_den as float32 arrays)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, F32))
    near, far = SC.cube_near_far(inp["rays_o"], inp["rays_d"], 1.6)
    mask = keep.astype(F32)
    up = {k: t(v * (mask if v.ndim == 1 else mask[:, None])) for k, v in inp["up"].items() if k != "eik"}
    up["eik"] = t(inp["up"]["eik"])
    N, T = saved["z_vals"].shape
    return dict(N=N, T0=c["T0"], T=T, car=B_CAR, weights="golden", group_rays=0, inv_s=torch.tensor([[inv_s]], dtype=torch.float32), rays_o=t(inp["rays_o"]),
                rays_d=t(inp["rays_d"]), near=t(near), far=t(far), bg=t(inp["bg"]), z=t(saved["z_vals"]), sdf=t(saved["sdf"]), color=t(saved["color"]),
                pts=t(saved["pts"]), gradient=t(saved["gradient"]), out16=t(saved["sdf_out16"]), eik_den=t(saved["eik_den"]).reshape(1), up=up)


def estimate_b(c):
    """the CPU tier's estimate of family B's zeroed share: the oracle's forward gives z_vals, sdf, gradient, color bit for bit; out16 comes from the
    float32 restatement -> (keep [N], the state)"""
    from oracle import oracle as O
    from tests.common import oracle_field_from_golden
    inp = inputs_b(c)
    inv_s = float(FC.params()["inv_s"])
    r = O.render_rays(oracle_field_from_golden(), inp["rays_o"], inp["rays_d"], c["T0"], c["up"], 1.6, inv_s, bg=inp["bg"], noise=inp["noise"])
    z = r["z_vals"]                                                        # the samples sit at the sections' middles (models/instant_nsr.py:197-204)
    z_mid = np.concatenate([z[:, :-1] + F32(0.5) * (z[:, 1:] - z[:, :-1]), z[:, -1:]], -1)
    pts = np.clip(inp["rays_o"][:, None, :] + inp["rays_d"][:, None, :] * z_mid[:, :, None], F32(-1.6), F32(1.6)).astype(F32)
    x = torch.from_numpy(pts.reshape(-1, 3))
    geo, Wt = geometry_f32(x.numpy(), "f32_mul_add"), weights_of("golden")
    feat, _ = encode(stencil_points(x), geo, torch.from_numpy(table_of("golden")[geo["rows"]]))
    out16, _ = sdf_query_ref(stencil_points(x), feat, *[Wt[k] for k in FC.SDF_W])
    N, T = r["z_vals"].shape
    out16 = out16.numpy().reshape(N, T, 16)
    keep = family_b_keep(pts, r["gradient"], out16, inp["rays_d"])
    relax = float((_norm32(pts) < F32(1.2)).sum()) + 1e-5
    saved = dict(z_vals=r["z_vals"], pts=pts, sdf=r["sdf"], sdf_out16=out16, gradient=r["gradient"], color=r["color"], eik_den=np.array([relax], F32))
    return keep, state_b(c, inp, saved, inv_s, keep)
