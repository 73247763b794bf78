"""-m gpu: training at the long renderer's counts (num_steps >= 2, upsample_steps a multiple of 16, at most 512 samples): the forward is
ac_render_rays_long with its per-sample outputs kept, the backward ac_render_core_backward with the long compositing kernels
(composite_*_kernel<512, true>) and the re-gathering SDF backward (no feat7).  Pinned against the reference's own gradients
(tests/golden/run_long_train.npz, run_long.npz), the fp64 oracle, the short route where both apply, and the autograd route of sds_step."""
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


def _case(gd, name):
    pre = name + "/"
    return {k[len(pre):]: v for k, v in gd.items() if k.startswith(pre)}


def _golden_net(train=False):
    from tests.test_gpu_model import golden_net
    return golden_net(train)


def _record(name, values):
    """the measured figures a bound below rests on, one JSON line on stdout (shown with -s, and with the failure report)"""
    print(json.dumps({name: values}))


def _manual_grads(net, out, ro, rd, bg, G, Gw, w_eik):
    """backward_last on a render_rays_long(train_extras=True) result: nsr_ops.render_core_backward + the parameters' own gradients"""
    net._last_train = (out, ro, rd, bg, net._field())
    net.backward_last(g_image=G, g_weights_sum=Gw, g_eik=torch.full((1,), float(w_eik), device=DEV))
    torch.cuda.synchronize()
    return {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}


# ---- 1. the reference's own gradients --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["train_128_128", "train_100_64", "train_256_0", "train_40_16", "run_long:train_96_32"])
def test_long_backward_matches_reference_gradients(name):
    from avatarcraft_amd import nsr_ops
    if name.startswith("run_long:"):
        c = _case(load_golden("run_long.npz"), name.split(":")[1])
        N = c["rays_o"].shape[0]
        G, Gw, w_eik = np.ones((N, 3), np.float32), None, 1.0                 # image.sum() + gradient_error
    else:
        c = _case(load_golden("run_long_train.npz"), name)
        G, Gw, w_eik = c["G"], c["Gw"], float(c["w_eik"])
    T0, up = int(c["num_steps"]), int(c["upsample_steps"])
    net, _ = _golden_net(train=True)
    ro, rd, bg = t(c["rays_o"]), t(c["rays_d"]), t(c["bg"])
    with torch.no_grad():
        out = nsr_ops.render_rays_long(net._field(), ro, rd, T0, up, 1.6, net.forward_variance(), bg=bg, noise=t(c["noise"]), extras=True,
                                       train_extras=True)
    assert out.get("feat7") is None
    assert np.abs(out["image"].cpu().numpy() - c["image"]).max() <= 1e-3
    if "weights_sum" in c:
        assert np.abs(out["weights_sum"].cpu().numpy() - c["weights_sum"]).max() <= 1e-3
    # The reference's sample_pdf decides some up-sampling indices by last-ulp comparisons (run_long.npz records such flips at 128 + 128): a ray whose
    # samples land elsewhere differentiates other points, so its case is held to a looser bound -- and only such a case.  Measured: 128 + 128 (z off
    # by 2.3e-3) 3.2e-3 of the largest entry, 100 + 64 (1.0e-4) 4.8e-3; the cases whose samples agree within 1e-4 stay within 1.8e-3.
    z_off = float(np.abs(out["z_vals"].cpu().numpy() - c["z_vals"]).max())
    tol = 3e-3 if z_off <= 1e-4 else 1e-2
    got = _manual_grads(net, out, ro, rd, bg, t(G), t(Gw), w_eik)
    worst = {"z_off": z_off}
    for k, g in got.items():
        if k == "encoder.embeddings":
            ref, g, scale = c["emb_grad"], g[c["emb_idx"]], float(c["emb_max"])
        else:
            ref = c["grad." + k]
            scale = float(np.abs(ref).max())
        worst[k] = float(np.abs(g - ref).max()) / (scale + 1e-30)
    _record("reference_" + name, worst)
    for k, e in worst.items():
        assert k == "z_off" or e <= tol, (k, e, worst)


# ---- 2. the fp64 oracle at ragged and long counts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T0,up", [(100, 16), (40, 16), (70, 48), (96, 32), (100, 64), (128, 128), (256, 0), (2, 496)])
def test_long_backward_matches_oracle_fp64(T0, up):
    from avatarcraft_amd import nsr_ops
    from oracle import oracle as O
    import bench
    p = load_golden("nsr_params.npz")
    f, table = device_field(p, device=DEV)
    of = oracle_field(p, table)
    ro, rd = bench.sds_view(0)                      # test_oracle_backward.py's 4096-ray patch
    if (T0, up) == (128, 128):
        # its first 1024 rays: with this case's upstream draws, d loss / d inv_s over the whole patch is a cancellation -- +0.168 on these rays,
        # -0.167 on the rest, a total of 1.4e-3 against 21.6 summed over the per-ray magnitudes -- so the relative bound below would measure
        # the cancellation (4.9e-3), not the backward (measured per part: 3.3e-5 and 7.4e-5 of the oracle's value)
        ro, rd = ro[:1024], rd[:1024]
    N = ro.shape[0]
    rs = np.random.RandomState(T0 * 1000 + up)
    noise = rs.uniform(0, 1, (N, T0)).astype(np.float32)
    bg = rs.uniform(0, 1, (N, 3)).astype(np.float32)
    g_img = np.clip(rs.normal(0, 1, (N, 3)), -1, 1).astype(np.float32)
    g_ws, g_dp, g_nm = rs.normal(0, 1, N).astype(np.float32), rs.normal(0, 1, N).astype(np.float32), rs.normal(0, 1, (N, 3)).astype(np.float32)
    g_eik, inv_s = 7.0, float(p["inv_s"])
    tro, trd, tbg = t(ro), t(rd), t(bg)
    out = nsr_ops.render_rays_long(f, tro, trd, T0, up, 1.6, inv_s, bg=tbg, noise=t(noise), extras=True, train_extras=True)
    g_table = torch.zeros_like(f.t["table"])
    g_sdf_p, g_col_p, g_invs = nsr_ops.render_core_backward(f, out.opts, out, tro, trd, tbg, t(g_img), t(g_ws), t(g_dp), t(g_nm),
                                                            torch.tensor(g_eik, device=DEV), g_table)
    torch.cuda.synchronize()
    g = dict(zip(("W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3"), nsr_ops.split_sdf_param_grads(g_sdf_p) + nsr_ops.split_color_param_grads(g_col_p)))
    z = out["z_vals"].cpu().numpy()
    r = O.render_core_backward(of, ro, rd, z, T0, up, 1.6, inv_s, bg=bg, g_image=g_img, g_weights_sum=g_ws, g_depth=g_dp, g_normal_map=g_nm, g_eik=g_eik)
    assert np.abs(r["image"] - out["image"].cpu().numpy()).max() <= 2e-5
    worst = {}
    for k, v in g.items():
        ref = r["g_" + k]
        worst[k] = float(np.abs(v.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
    worst["inv_s"] = abs(float(g_invs.sum()) - r["g_inv_s"]) / abs(r["g_inv_s"])
    touched = np.flatnonzero(np.abs(r["g_table"]).sum(1))
    pick = touched[np.random.RandomState(4).choice(len(touched), min(65536, len(touched)), replace=False)]
    gt = g_table[torch.from_numpy(pick).to(DEV)].cpu().numpy().astype(np.float64)
    worst["table"] = float(np.abs(gt - r["g_table"][pick]).max() / np.abs(r["g_table"]).max())
    _record(f"oracle_{T0}_{up}", worst)
    # test_oracle_backward.py's tolerance (exact arithmetic) for everything the compositing backward feeds directly (inv_s, Wc3) and for the SDF side
    # (measured <= 1.2e-4).  The colour network's first two layers are further off here: measured 4.3e-4 - 3.3e-3 of the largest entry (Wc1 at 40 + 16,
    # Wc2 up to 1.9e-3), 96 + 32 (T = 128, no ragged tile) included.  That is not the arithmetic of color_bwd_kernel: it is ReLU gates that flip against
    # a float64 oracle.  The oracle decides the 128 gates of a sample from its own float64 pre-activations, the kernel from the float32 ones the forward
    # saw, and on 4096 rays some thousand samples have a unit within float32 rounding of zero; a flipped gate moves a whole row's share of d Wc1 / d Wc2.
    # With the gates shared -- the chain of vector-Jacobian products at the saved float32 state, rays with a pre-activation within 2^-16 of its terms'
    # absolute sum zeroed upstream (tests/test_gpu_core_backward.py, family B, these kernels at 16 + 16, 32 + 32 and 40 + 16) -- d Wc1 is within 2.8e-6
    # and d Wc2 within 1.3e-6 of the largest entry of float64 autograd: 0.84 and 0.66 times the float32 restatement's own error.
    for k, e in worst.items():
        assert e <= (5e-3 if k in ("Wc1", "Wc2") else 3e-4), (k, e, worst)


# ---- 3. where both routes apply: the long route's backward (no feat7) against the short one's (render_rays + feat7) ------------------------------
# The compositing and colour backward are the same kernels on the same bits (the long forward equals the short one bit for bit), so g_color_params and
# g_inv_s_per_ray agree exactly.  The SDF backward is not the same arithmetic: the saved-feature form (sdf_stencil_bwd_kernel<SAVED = true>) forms the
# weight-gradient products d1 inp^T on the bf16 matrix pipe (split bf16, halves rounded to nearest) and deals the tiles to its own number of waves per
# workgroup, so the bits of g_sdf_params (and of g_table, wherever the two forms' per-sample arithmetic differs) are not the same.  Bound: see the
# assertions and the measured figures they record.
@pytest.mark.parametrize("T0,up", [(32, 32), (64, 64), (48, 80)])
def test_long_route_backward_equals_short_route(T0, up):
    from avatarcraft_amd import nsr_ops
    p = load_golden("nsr_params.npz")
    f, _ = device_field(p, device=DEV)
    ro, rd = make_rays(32, 32, dist=1.7, f=25.0)
    N = ro.shape[0]
    rs = np.random.RandomState(5)
    noise, bg = t(rs.uniform(0, 1, (N, T0))), t(rs.uniform(0, 1, (N, 3)))
    g_img, g_ws = t(rs.normal(0, 1, (N, 3))), t(rs.normal(0, 1, N))
    tro, trd = t(ro), t(rd)
    res = {}
    for route, render in (("short", nsr_ops.render_rays), ("long", nsr_ops.render_rays_long)):
        out = render(f, tro, trd, T0, up, 1.6, float(p["inv_s"]), bg=bg, noise=noise, extras=True, train_extras=True)
        assert ("feat7" in out) == (route == "short")
        g_table = torch.zeros_like(f.t["table"])
        g_sdf_p, g_col_p, g_invs = nsr_ops.render_core_backward(f, out.opts, out, tro, trd, bg, g_img, g_ws, None, None,
                                                                torch.tensor(0.01, device=DEV), g_table)
        torch.cuda.synchronize()
        res[route] = dict(g_table=g_table, g_sdf_params=g_sdf_p, g_color_params=g_col_p, g_inv_s_per_ray=g_invs, image=out["image"].clone())
    a, b = res["long"], res["short"]
    assert torch.equal(a["image"], b["image"])
    assert torch.equal(a["g_color_params"], b["g_color_params"])
    assert torch.equal(a["g_inv_s_per_ray"], b["g_inv_s_per_ray"])
    rel = {k: float((a[k] - b[k]).abs().max()) / float(b[k].abs().max()) for k in ("g_table", "g_sdf_params")}
    rel["g_table_bitwise"] = bool(torch.equal(a["g_table"], b["g_table"]))
    rel["g_sdf_params_bitwise"] = bool(torch.equal(a["g_sdf_params"], b["g_sdf_params"]))
    _record(f"overlap_{T0}_{up}", rel)
    assert rel["g_table_bitwise"], rel                                      # the data gradient (gfeat) is the same per sample
    assert rel["g_sdf_params"] <= 1e-4, rel                                # measured 6.9e-5 (32 + 32), 4.9e-6 (64 + 64), 7.8e-6 (48 + 80)


# ---- the long compositing kernels: the long forward's weights bit for bit; the short ones still where they apply --------------------------------
@pytest.mark.parametrize("T0,up", [(100, 64), (40, 16), (128, 128), (256, 0), (37, 0), (32, 32), (64, 64)])
def test_composite_forward_equals_the_renderers_weights(T0, up):
    from avatarcraft_amd import nsr_ops
    p = load_golden("nsr_params.npz")
    f, _ = device_field(p, device=DEV)
    ro, rd = make_rays(16, 16, dist=1.7, f=12.0)
    N = ro.shape[0]
    rs = np.random.RandomState(6)
    noise, bg = t(rs.uniform(0, 1, (N, T0))), t(rs.uniform(0, 1, (N, 3)))
    tro, trd = t(ro), t(rd)
    out = nsr_ops.render_rays_long(f, tro, trd, T0, up, 1.6, float(p["inv_s"]), bg=bg, noise=noise, extras=True)
    g = out["gradient"].cpu().numpy()                                     # normals as core_normals_kernel forms them (fp32, correctly rounded)
    gn = np.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])
    nrm = t(g / (np.float32(1e-5) + gn)[..., None])
    inv_s = torch.tensor([float(p["inv_s"])], device=DEV)
    image, wsum, depth, nmap, weights, alpha = nsr_ops.composite(out["z_vals"], out["sdf"], nrm, out["color"], inv_s, tro, trd, bg, T0, 1.6, 1.0)
    for k, v in (("weights", weights), ("alpha", alpha), ("image", image), ("weights_sum", wsum), ("normal_map", nmap)):
        assert torch.equal(v, out[k]), k
    assert torch.equal(depth, out["depth"])


# ---- 4. sds_step at long counts: the fused route against the autograd route -------------------------------------------------------------------------
def _sds(manual, T0, up, route, seed=11):
    from avatarcraft_amd.stylize import sds_step, SyntheticGuidance, flat_grad_view

    class Shared(SyntheticGuidance):
        private_rng = False                 # a guidance that draws from the global streams: the reference's order, no pair launch

    net, _ = _golden_net(train=True)
    net_gt, _ = _golden_net(train=False)
    if not manual:
        net.manual_backward_supported = lambda *a, **k: False
    if route == "view":
        ro, rd, hw, bs = *make_rays(64, 32, dist=1.8, f=40.0), (64, 32), 512
    else:
        ro, rd, hw, bs = *make_rays(16, 16, dist=1.8, f=10.0), (16, 16), 4096
    guide = Shared(5) if route == "shared" else SyntheticGuidance(5)
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    flat = flat_grad_view(net.parameters())
    marks = []
    torch.manual_seed(seed)
    stats = sds_step(net, net_gt, t(ro), t(rd), hw, opt, guide, batch_size=bs, flat_grad=flat, num_steps=T0, upsample_steps=up, timers=marks)
    torch.cuda.synchronize()
    net.check_finite()
    return ({k: v.grad.detach().clone() for k, v in net.named_parameters()}, {k: v.detach().clone() for k, v in net.named_parameters()}, stats,
            [n for n, _ in marks])


@pytest.mark.parametrize("route", ["pair", "shared", "view"])
@pytest.mark.parametrize("T0,up", [(128, 128), (100, 64)])
def test_sds_step_at_long_counts_equals_autograd_step(T0, up, route):
    g1, p1, s1, m1 = _sds(True, T0, up, route)
    g0, p0, s0, m0 = _sds(False, T0, up, route)
    if route == "pair":
        assert "render_val_and_grad_forward" in m1                         # the pair route (two launches of the long renderer)
    worst = {}
    for k in g0:
        scale = float(g0[k].abs().max())
        assert scale > 0, k
        worst[k] = float((g1[k] - g0[k]).abs().max()) / scale
        clear = g0[k].abs() > 1e-2 * scale                                  # Adam's first step is lr * sign(g): compared where the sign is clear
        assert float((p1[k] - p0[k])[clear].abs().max()) <= 1e-6, k
    _record(f"sds_{route}_{T0}_{up}", worst)
    # the autograd route's render core at these counts is torch glue over the fused SDF / colour operators, not one fused operator as at 64 + 64
    # (test_gpu_model.py: 2e-5): measured at most 2.2e-4 of the largest entry (128 + 128, sdf_net.1.weight_g), 2.4e-5 at 100 + 64
    for k, e in worst.items():
        assert e <= 5e-4, (k, e, worst)
    assert abs(float(s1["opacity"]) - float(s0["opacity"])) <= 1e-4 * abs(float(s0["opacity"])) + 1e-6
    assert abs(float(s1["eikonal"]) - float(s0["eikonal"])) <= 1e-4 * abs(float(s0["eikonal"])) + 1e-9
    g2, p2, _, _ = _sds(True, T0, up, route)                             # two identical steps: identical bits
    for k in g1:
        assert torch.equal(g1[k], g2[k]) and torch.equal(p1[k], p2[k]), k


# ---- 5. the whole-view backward at 128 + 128 ------------------------------------------------------------------------------------------------------
def test_whole_view_backward_at_long_count_equals_patch_by_patch():
    import avatarcraft_amd.stylize as ST
    ro, rd = make_rays(64, 32, dist=1.8, f=40.0)                          # 2048 rays: 4 patches of 512
    ro_t, rd_t = t(ro), t(rd)

    class Rec(ST.SyntheticGuidance):
        def __call__(self, rgb, text=None):
            self.seen = rgb.detach().clone()
            return super().__call__(rgb, text)

    def one(whole):
        net, _ = _golden_net(train=True)
        net_gt, _ = _golden_net(train=False)
        opt = torch.optim.SGD(net.parameters(), lr=0.0)
        flat = ST.flat_grad_view(net.parameters())
        guide = Rec(3)
        torch.manual_seed(21)
        marks = []
        prev = ST.WHOLE_VIEW_BACKWARD
        ST.WHOLE_VIEW_BACKWARD = whole
        try:
            st = ST.sds_step(net, net_gt, ro_t, rd_t, (64, 32), opt, guide, batch_size=512, flat_grad=flat, num_steps=128, upsample_steps=128, timers=marks)
        finally:
            ST.WHOLE_VIEW_BACKWARD = prev
        net.check_finite()
        return guide.seen, {k: v.grad.detach().clone() for k, v in net.named_parameters()}, [n for n, _ in marks], st
    img_a, g_a, m_a, s_a = one(True)
    img_b, g_b, m_b, s_b = one(False)
    assert m_a.count("backward") == 1 and m_b.count("backward") == 4
    assert torch.equal(img_a, img_b)
    assert abs(float(s_a["opacity"]) - float(s_b["opacity"])) <= 1e-6 * abs(float(s_b["opacity"]))
    assert abs(float(s_a["eikonal"]) - float(s_b["eikonal"])) <= 1e-6 * abs(float(s_b["eikonal"]))
    worst = {}
    for k in g_a:
        scale = float(g_b[k].abs().max())
        assert scale > 0, k
        worst[k] = float((g_a[k] - g_b[k]).abs().max()) / scale
    _record("whole_view_128_128", worst)
    for k, e in worst.items():
        assert e <= 5e-6, (k, e, worst)                                    # test_gpu_stylize.py's bound at 64 + 64


# ---- 6. view directions ---------------------------------------------------------------------------------------------------------------------------
def _sds_vd(manual, T0, up):
    from avatarcraft_amd.stylize import sds_step, SyntheticGuidance, flat_grad_view
    from tests.test_gpu_viewdirs import viewdirs_net
    g = load_golden("viewdirs.npz")
    ro, rd = make_rays(16, 16, dist=1.8, f=10.0)
    net, net_gt = viewdirs_net(g, train=True), viewdirs_net(g)
    if not manual:
        net.manual_backward_supported = lambda *a, **k: False
    opt = torch.optim.Adam(net.parameters(), lr=5e-3)
    flat = flat_grad_view(net.parameters())
    torch.manual_seed(3)
    sds_step(net, net_gt, t(ro), t(rd), (16, 16), opt, SyntheticGuidance(5), batch_size=4096, flat_grad=flat, num_steps=T0, upsample_steps=up)
    torch.cuda.synchronize()
    net.check_finite()
    return net, {k: v.grad.detach().clone() for k, v in net.named_parameters()}


def test_viewdirs_at_long_counts():
    net, ga = _sds_vd(True, 96, 32)                                     # T = 128: the fused manual backward with the view-direction bias
    assert net.manual_backward_supported(96, 32)
    _, gb = _sds_vd(False, 96, 32)
    worst = {}
    for k in ga:
        scale = float(gb[k].abs().max())
        worst[k] = float((ga[k] - gb[k]).abs().max()) / (scale + 1e-30)
    _record("viewdirs_96_32", worst)
    for k, e in worst.items():                                          # measured at most 8.6e-5 (deviation_net.variance)
        assert e <= 5e-4, (k, e, worst)
    assert float(ga["color_net.0.weight_v"][:, 3:19].abs().max()) > 0
    net, gc = _sds_vd(True, 100, 64)                                    # T = 164: not for the fused backward; sds_step takes the autograd loop
    assert net.manual_backward_supported() and not net.manual_backward_supported(100, 64)
    _, gd = _sds_vd(False, 100, 64)
    for k in gc:                                                        # the same route twice (its hash backward sums with atomics: last bits)
        assert torch.isfinite(gc[k]).all(), k
        assert float((gc[k] - gd[k]).abs().max()) <= 1e-5 * float(gd[k].abs().max()) + 1e-12, k


# ---- 7. the rules -----------------------------------------------------------------------------------------------------------------------------------
def test_long_backward_rules():
    from avatarcraft_amd import nsr_ops
    p = load_golden("nsr_params.npz")
    f, _ = device_field(p, device=DEV)
    ro, rd = make_rays(4, 4, dist=1.7)
    tro, trd = t(ro), t(rd)
    out = nsr_ops.render_rays_long(f, tro, trd, 100, 16, 1.6, float(p["inv_s"]), extras=True, train_extras=True)
    out["feat7"] = torch.zeros((16 * 116 // 16 + 1, 14, 64, 4), device=DEV)
    with pytest.raises(RuntimeError, match="feat7 needs T a multiple of 16"):
        nsr_ops.render_core_backward(f, out.opts, out, tro, trd, None, torch.ones((16, 3), device=DEV), None, None, None, None, torch.zeros_like(f.t["table"]))
    Wsh = t(np.random.RandomState(41).normal(0.0, 0.2, (64, 16)).astype(np.float32))
    fvd = nsr_ops.Field(f.t["table"], [int(v) for v in p["offsets"]], float(p["per_level_scale"]), 16, f.t["W1"], f.t["b1"], f.t["W2"], f.t["b2"],
                        f.t["Wc1"], f.t["Wc2"], f.t["Wc3"], Wc1_sh=Wsh)
    out = nsr_ops.render_rays_long(fvd, tro, trd, 100, 16, 1.6, float(p["inv_s"]), extras=True, train_extras=True)
    with pytest.raises(RuntimeError, match="view directions needs T a multiple of 16"):
        nsr_ops.render_core_backward(fvd, out.opts, out, tro, trd, None, torch.ones((16, 3), device=DEV), None, None, None, None, torch.zeros_like(f.t["table"]))
    z = torch.zeros((16, 528), device=DEV)
    n3 = torch.zeros((16, 528, 3), device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        nsr_ops.composite(z, z, n3, n3, torch.ones(1, device=DEV), tro, trd, None, 16, 1.6, 1.0)
