"""-m gpu: the training options of the long renderer in canonical space: the stencil features feat7 (save_stencil), the pair
launch (ac_render_rays_long_pair) and opacity_only, and the model switch NeRFNetwork.long_step_extras that routes stylize.sds_step to them.
Yardsticks: the short kernel's own feat7 and gradients inside its window (bit for bit), the fp64 oracle at long counts, two separate launches for the
pair, the full render for opacity_only, the autograd step for sds_step.  CPU tier: tests/test_long_step_extras_host.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests.common import load_golden, make_rays
from tests.gpu_common import device_field, oracle_field

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _record(name, values):
    """the measured figures a bound below rests on, one JSON line on stdout (shown with -s, and with the failure report)"""
    print(json.dumps({name: values}))


_FIELD = {}


def _field():
    """the golden field, made once for the module (read-only)"""
    if not _FIELD:
        p = load_golden("nsr_params.npz")
        f, table = device_field(p, device=DEV)
        _FIELD.update(p=p, f=f, table=table, inv_s=float(p["inv_s"]))
    return _FIELD


def _rays(h=9, w=9):
    """81 rays: no multiple of 7 (the long kernel's waves per workgroup) or 8 -- the last workgroup is ragged; odd, for the pair"""
    ro, rd = make_rays(h, w, dist=1.7, f=1.6 * w)
    return t(ro), t(rd), ro, rd


def _inputs(N, T0, seed):
    rs = np.random.RandomState(seed)
    return dict(noise=t(rs.uniform(0, 1, (N, T0))), bg=t(rs.uniform(0, 1, (N, 3))), g_img=t(rs.normal(0, 1, (N, 3))), g_ws=t(rs.normal(0, 1, N)))


def _backward(f, out, ro, rd, bg, g_img, g_ws, g_dp=None, g_nm=None, g_eik=0.01):
    from avatarcraft_amd import nsr_ops
    g_table = torch.zeros_like(f.t["table"])
    g_sdf_p, g_col_p, g_invs = nsr_ops.render_core_backward(f, out.opts, out, ro, rd, bg, g_img, g_ws, g_dp, g_nm, torch.tensor(g_eik, device=DEV), g_table)
    torch.cuda.synchronize()
    return dict(g_table=g_table, g_sdf_params=g_sdf_p, g_color_params=g_col_p, g_inv_s_per_ray=g_invs, image=out["image"].clone())


# ---- 1 + 2. inside the window: the short kernel's feat7 bit for bit, and with it the short route's gradients bit for bit ----------------------------
@pytest.mark.parametrize("precision", ["exact", "fast"])
@pytest.mark.parametrize("T0,up", [(32, 32), (64, 64), (48, 80)])
def test_feat7_and_gradients_equal_the_short_route(T0, up, precision):
    from avatarcraft_amd import nsr_ops
    e = _field()
    ro, rd, _, _ = _rays()
    x = _inputs(ro.shape[0], T0, 5)
    kw = dict(bg=x["bg"], noise=x["noise"], extras=True, train_extras=True, precision=precision)
    short = nsr_ops.render_rays(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], **kw)
    long_ = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], save_stencil=True, **kw)
    assert long_["feat7"].shape == short["feat7"].shape == (ro.shape[0] * (T0 + up) // 16, 14, 64, 4)
    assert float(short["feat7"].abs().max()) > 0
    assert torch.equal(long_["feat7"], short["feat7"])
    # the default stays without the features, and a reused result dict drops another launch's
    again = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], out=long_, **kw)
    assert again.get("feat7") is None
    long_ = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], save_stencil=True, **kw)
    a = _backward(e["f"], long_, ro, rd, x["bg"], x["g_img"], x["g_ws"])
    b = _backward(e["f"], short, ro, rd, x["bg"], x["g_img"], x["g_ws"])
    for k in ("g_table", "g_sdf_params", "g_color_params", "g_inv_s_per_ray", "image"):      # the same form of the backward on the same bits
        assert torch.equal(a[k], b[k]), k
    assert float(b["g_sdf_params"].abs().max()) > 0 and float(b["g_table"].abs().max()) > 0


# ---- 3. long counts: the backward from the saved features against the fp64 oracle, and against the re-gathering form ---------------------------------
# Bounds: test_long_backward_matches_oracle_fp64's (3e-4 of each tensor's largest entry, 5e-3 for Wc1 / Wc2), and for the two forms of the SDF backward
# test_long_route_backward_equals_short_route's 1e-4 of the largest entry.  The upstream gradient of weights_sum is one-signed here (|normal| draws): the
# oracle test records that d loss / d inv_s over a batch can be a cancellation between rays, and a relative bound on a sum only measures the backward
# when the sum is not one.
@pytest.mark.parametrize("T0,up", [(128, 128), (96, 32), (16, 496)])
def test_saved_features_backward_matches_oracle_fp64(T0, up):
    from avatarcraft_amd import nsr_ops
    from oracle import oracle as O
    e = _field()
    of = oracle_field(e["p"], e["table"])
    tro, trd, ro, rd = _rays()
    N = ro.shape[0]
    rs = np.random.RandomState(T0 * 1000 + up)
    noise = rs.uniform(0, 1, (N, T0)).astype(np.float32)
    bg = rs.uniform(0, 1, (N, 3)).astype(np.float32)
    g_img = np.clip(rs.normal(0, 1, (N, 3)), -1, 1).astype(np.float32)
    g_ws, g_dp, g_nm = np.abs(rs.normal(0, 1, N)).astype(np.float32), rs.normal(0, 1, N).astype(np.float32), rs.normal(0, 1, (N, 3)).astype(np.float32)
    g_eik, inv_s = 7.0, e["inv_s"]
    tbg = t(bg)
    res = {}
    for form, save in (("saved", True), ("gather", False)):
        out = nsr_ops.render_rays_long(e["f"], tro, trd, T0, up, 1.6, inv_s, bg=tbg, noise=t(noise), extras=True, train_extras=True, save_stencil=save)
        assert ("feat7" in out) == save
        res[form] = _backward(e["f"], out, tro, trd, tbg, t(g_img), t(g_ws), t(g_dp), t(g_nm), g_eik)
        res[form]["z"] = out["z_vals"].cpu().numpy()
    a, b = res["saved"], res["gather"]
    assert np.array_equal(a["z"], b["z"]) and torch.equal(a["image"], b["image"])
    r = O.render_core_backward(of, ro, rd, a["z"], T0, up, 1.6, inv_s, bg=bg, g_image=g_img, g_weights_sum=g_ws, g_depth=g_dp, g_normal_map=g_nm, g_eik=g_eik)
    assert np.abs(r["image"] - a["image"].cpu().numpy()).max() <= 2e-5
    worst = {}
    for form, x in res.items():
        g_sdf_p, g_col_p = x["g_sdf_params"], x["g_color_params"]
        g = dict(zip(("W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3"), nsr_ops.split_sdf_param_grads(g_sdf_p) + nsr_ops.split_color_param_grads(g_col_p)))
        w = {k: float(np.abs(v.cpu().numpy().astype(np.float64) - r["g_" + k]).max() / np.abs(r["g_" + k]).max()) for k, v in g.items()}
        w["inv_s"] = abs(float(x["g_inv_s_per_ray"].sum()) - r["g_inv_s"]) / abs(r["g_inv_s"])
        w["table"] = float(np.abs(x["g_table"].cpu().numpy().astype(np.float64) - r["g_table"]).max() / np.abs(r["g_table"]).max())
        worst[form] = w
    forms = {k: float((a[k] - b[k]).abs().max()) / float(b[k].abs().max()) for k in ("g_table", "g_sdf_params")}
    forms.update({k + "_bitwise": bool(torch.equal(a[k], b[k])) for k in ("g_table", "g_color_params", "g_inv_s_per_ray")})
    worst["saved_vs_gather"] = forms
    _record(f"saved_oracle_{T0}_{up}", worst)
    for k, err in worst["saved"].items():
        assert err <= (5e-3 if k in ("Wc1", "Wc2") else 3e-4), (k, err, worst)
    assert forms["g_table_bitwise"] and forms["g_color_params_bitwise"] and forms["g_inv_s_per_ray_bitwise"], forms
    assert forms["g_sdf_params"] <= 1e-4, forms


# ---- 4. the pair launch equals two launches -------------------------------------------------------------------------------------------------------------
PER_RAY = ("image", "weights_sum", "depth", "normal_map", "eik")
PER_SAMPLE = ("z_vals", "color", "sdf", "gradient", "sdf_out16", "pts", "weights", "alpha")


def _pair_case(T0, up, ro, rd, precision="exact"):
    from avatarcraft_amd import nsr_ops
    e = _field()
    N, T = ro.shape[0], T0 + up
    rs = np.random.RandomState(17 + T0)
    noise2, bg2 = t(rs.uniform(0, 1, (2, N, T0))), t(rs.uniform(0, 1, (2, N, 3)))
    save = T % 16 == 0
    kw = dict(precision=precision)
    ra, rb = nsr_ops.render_rays_long_pair(e["f"], ro, rd, noise2, T0, up, 1.6, e["inv_s"], bg2=bg2, keep_weights=True, save_stencil=save, **kw)
    one = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], bg=bg2[0], noise=noise2[0], **kw)
    two = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], bg=bg2[1], noise=noise2[1], extras=True, train_extras=True, save_stencil=save, **kw)
    torch.cuda.synchronize()
    for k in PER_RAY:
        assert ra[k].shape == one[k].shape and torch.equal(ra[k], one[k]), ("copy a", k)
        assert torch.equal(rb[k], two[k]), ("copy b", k)
    for k in PER_SAMPLE:
        assert rb[k].shape == two[k].shape and torch.equal(rb[k], two[k]), k
    assert ("feat7" in rb) == save and ("feat7" in two) == save
    if save:
        assert torch.equal(rb["feat7"], two["feat7"]) and float(two["feat7"].abs().max()) > 0
    assert torch.equal(ra["eik_res"], one["eik_res"]) and torch.equal(rb["eik_res"], two["eik_res"])
    assert torch.equal(ra["gradient_error"], one["gradient_error"]) and torch.equal(rb["gradient_error"], two["gradient_error"])
    assert not torch.equal(ra["image"], rb["image"])                      # two draws: two different renders
    return rb, two


@pytest.mark.parametrize("T0,up", [(64, 64), (100, 64), (37, 0), (128, 128)])
def test_pair_equals_two_launches(T0, up):
    ro, rd, _, _ = _rays()
    rb, two = _pair_case(T0, up, ro, rd, precision="fast" if (T0, up) == (100, 64) else "exact")
    if (T0 + up) % 16 == 0:                                                # copy b feeds the backward like a launch of its own
        e = _field()
        x = _inputs(ro.shape[0], T0, 9)
        bg = rb._keep[1][ro.shape[0]:]
        a, b = _backward(e["f"], rb, ro, rd, bg, x["g_img"], x["g_ws"]), _backward(e["f"], two, ro, rd, bg, x["g_img"], x["g_ws"])
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("h,w", [(1, 1), (27, 19)])
def test_pair_at_one_ray_and_across_a_chunk_boundary(h, w):
    """N = 1: one chunk of two work items; N = 513: 1026 work items, the copies of the rays around 256 sit on both sides of a 512-item chunk boundary and
    the last chunk holds two items"""
    ro, rd, _, _ = _rays(h, w)
    assert ro.shape[0] in (1, 513)
    _pair_case(48, 16, ro, rd)


# ---- 5. opacity_only ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T0,up", [(100, 64), (128, 128), (64, 64)])
def test_opacity_only_changes_the_image_alone(T0, up):
    from avatarcraft_amd import nsr_ops
    e = _field()
    ro, rd, _, _ = _rays()
    x = _inputs(ro.shape[0], T0, 23)
    kw = dict(bg=x["bg"], noise=x["noise"], extras=True)
    full = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], **kw)
    opa = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], opacity_only=True, **kw)
    lean = nsr_ops.render_rays_long(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], bg=x["bg"], noise=x["noise"], opacity_only=True)     # the frozen avatar's launch
    for k in ("weights_sum", "depth", "normal_map", "eik", "z_vals", "weights", "alpha", "sdf", "gradient", "gradient_error"):
        assert torch.equal(opa[k], full[k]), k
    for k in ("weights_sum", "depth", "normal_map", "eik", "image", "gradient_error"):
        assert torch.equal(lean[k], opa[k]), k
    assert float(full["weights_sum"].max()) > 0.5                            # the body is in the picture
    # the background over a black body, formed as the kernels form it: s_rgb + (1 - s_w) * bg with s_rgb = +0
    want = torch.zeros_like(x["bg"]) + (1.0 - full["weights_sum"])[:, None] * x["bg"]
    assert torch.equal(opa["image"], want)
    assert not torch.equal(opa["image"], full["image"]) and float(opa["color"].abs().max()) == 0.0
    if nsr_ops.in_short_window(T0, up):
        short = nsr_ops.render_rays(e["f"], ro, rd, T0, up, 1.6, e["inv_s"], opacity_only=True, **kw)
        for k in ("image", "weights_sum", "depth", "normal_map", "eik", "z_vals", "weights", "alpha", "color", "sdf", "gradient"):
            assert torch.equal(opa[k], short[k]), k


# ---- 6. the rules ---------------------------------------------------------------------------------------------------------------------------------------------
def test_rules_on_the_device():
    from avatarcraft_amd import nsr_ops, _lib as L
    e = _field()
    ro, rd, _, _ = _rays(3, 3)
    with pytest.raises(RuntimeError, match=r"save_stencil \(feat7\) needs num_steps \+ upsample_steps a multiple of 16"):
        nsr_ops.render_rays_long(e["f"], ro, rd, 100, 64, 1.6, e["inv_s"], extras=True, train_extras=True, save_stencil=True)
    with pytest.raises(RuntimeError, match="table_dtype='half'"):
        nsr_ops.render_rays_long(e["f"], ro, rd, 128, 128, 1.6, e["inv_s"], train_extras=True, save_stencil=True, table_dtype="half")
    with pytest.raises(RuntimeError, match="opacity_only"):
        nsr_ops.render_rays_long(e["f"], ro, rd, 100, 64, 1.6, e["inv_s"], warp=object(), opacity_only=True)
    # the raw entries at T = 164 with feat7 set: refused, naming the rule; nothing is written
    N = ro.shape[0]
    lin_z, lin_u = nsr_ops.linspace_tables(100, ro.device)
    bufs = {k: torch.zeros(s, device=DEV) for k, s in (("image", (2 * N, 3)), ("weights_sum", (2 * N,)), ("depth", (2 * N,)), ("normal_map", (2 * N, 3)),
                                                        ("eik", (2 * N, 2)), ("feat7", (N * 164 // 16 + 1, 14, 64, 4)))}
    o = L.ac_render_out()
    for k, v in bufs.items():
        setattr(o, k, v.data_ptr())
    op = L.ac_render_opts(N, 100, 64, 1.6, e["inv_s"], 1.0, 0.005, 0, None, None, None, 0, 0, 0)
    for entry in (L.lib().ac_render_rays_long, L.lib().ac_render_rays_long_pair):
        rc = entry(C.byref(e["f"].c), C.byref(op), ro.data_ptr(), rd.data_ptr(), None, None, lin_z.data_ptr(), lin_u.data_ptr(), C.byref(o), L.current_stream(ro.device))
        assert rc != 0 and b"feat7" in L.lib().ac_last_error() and b"multiple of 16" in L.lib().ac_last_error()
    torch.cuda.synchronize()
    assert float(bufs["feat7"].abs().max()) == 0.0 and float(bufs["image"].abs().max()) == 0.0


# ---- 6 + 7. the step: NeRFNetwork.long_step_extras --------------------------------------------------------------------------------------------------------
def _sds(T0, up, route, extras, seed=11):
    """tests/test_gpu_long_train.py's _sds (one sds_step on the golden net, fused route) with the switch set -- extras None: never touched"""
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.stylize import sds_step, SyntheticGuidance, flat_grad_view
    from tests.test_gpu_model import golden_net

    class Shared(SyntheticGuidance):
        private_rng = False                 # a guidance that draws from the global streams: the reference's order, no pair launch

    net, _ = golden_net(True)
    net_gt, _ = golden_net(False)
    if extras is not None:
        net.long_step_extras = net_gt.long_step_extras = extras
    if route in ("view", "whole"):
        ro, rd, hw, bs = *make_rays(64, 32, dist=1.8, f=40.0), (64, 32), 512
    else:
        ro, rd, hw, bs = *make_rays(16, 16, dist=1.8, f=10.0), (16, 16), 4096
    guide = Shared(5) if route == "shared" else SyntheticGuidance(5)
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    flat = flat_grad_view(net.parameters())
    calls = []
    spy = {}
    for name in ("render_rays_long", "render_rays_long_pair"):
        def wrap(*a, _f=getattr(nsr_ops, name), _n=name, **k):
            r = _f(*a, **k)
            last = r[1] if isinstance(r, tuple) else r
            calls.append((_n, bool(k.get("opacity_only")), "feat7" in last, bool(k.get("train_extras")) or isinstance(r, tuple)))
            return r
        spy[name] = getattr(nsr_ops, name)
        setattr(nsr_ops, name, wrap)
    import avatarcraft_amd.stylize as ST
    prev = ST.WHOLE_VIEW_BACKWARD
    ST.WHOLE_VIEW_BACKWARD = prev or route == "whole"
    try:
        torch.manual_seed(seed)
        stats = sds_step(net, net_gt, t(ro), t(rd), hw, opt, guide, batch_size=bs, flat_grad=flat, num_steps=T0, upsample_steps=up)
    finally:
        ST.WHOLE_VIEW_BACKWARD = prev
        for name, f in spy.items():
            setattr(nsr_ops, name, f)
    torch.cuda.synchronize()
    net.check_finite()
    return ({k: v.grad.detach().clone() for k, v in net.named_parameters()}, {k: v.detach().clone() for k, v in net.named_parameters()}, stats, calls)


def test_switch_off_changes_nothing():
    g0, p0, _, c0 = _sds(128, 128, "pair", None)
    g1, p1, _, c1 = _sds(128, 128, "pair", False)
    assert c0 == c1 and [c[0] for c in c0].count("render_rays_long_pair") == 0
    assert not any(c[1] or c[2] for c in c0)                               # no opacity_only, no feat7: today's routes
    for k in p0:
        assert torch.equal(p0[k], p1[k]) and torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("T0,up,route", [(128, 128, "pair"), (128, 128, "shared"), (96, 32, "pair"), (96, 32, "shared"), (96, 32, "view"), (96, 32, "whole"), (100, 64, "pair")])
def test_sds_step_with_the_switch_equals_autograd_step(T0, up, route):
    from tests.test_gpu_long_train import _sds as sds_reference
    g1, p1, s1, calls = _sds(T0, up, route, True)
    g0, p0, s0, _ = sds_reference(False, T0, up, "view" if route == "whole" else route)      # the autograd step
    whole = (T0 + up) % 16 == 0
    train = [c for c in calls if c[3]]
    if route == "view":                                                     # 4 patches of 512 rays, patch by patch through run(): as inside the window, each keeps its features
        assert len(train) == 4 and all(c[0] == "render_rays_long" and c[2] == whole for c in train)
    elif route == "pair":
        assert len(train) == 1
        assert train[0][0] == "render_rays_long_pair" and train[0][2] == whole      # one launch; feat7 only where 16 | T
    elif route == "shared":
        assert len(train) == 1
        assert train[0][0] == "render_rays_long" and train[0][2] == whole
    else:                                                                   # stylize.WHOLE_VIEW_BACKWARD: one training render of the view (render_view_train)
        assert len(train) == 1
        assert train[0][0] == "render_rays_long" and not train[0][2]                 # ... which keeps re-gathering
    frozen = [c for c in calls if c[1]]
    assert len(frozen) == 1 and not frozen[0][3]                                     # the frozen avatar: one opacity_only launch
    worst = {}
    for k in g0:
        scale = float(g0[k].abs().max())
        assert scale > 0, k
        worst[k] = float((g1[k] - g0[k]).abs().max()) / scale
        clear = g0[k].abs() > 1e-2 * scale                                  # Adam's first step is lr * sign(g): compared where the sign is clear
        assert float((p1[k] - p0[k])[clear].abs().max()) <= 1e-6, k
    _record(f"sds_extras_{route}_{T0}_{up}", worst)
    for k, err in worst.items():                                            # test_sds_step_at_long_counts_equals_autograd_step's bounds
        assert err <= 5e-4, (k, err, worst)
    assert abs(float(s1["opacity"]) - float(s0["opacity"])) <= 1e-4 * abs(float(s0["opacity"])) + 1e-6
    assert abs(float(s1["eikonal"]) - float(s0["eikonal"])) <= 1e-4 * abs(float(s0["eikonal"])) + 1e-9
