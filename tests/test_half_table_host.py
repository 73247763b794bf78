"""CPU tier of the half-precision hash table (ac_table_to_half, ac_render_rays_h16, ac_render_rays_warped_h16; GPU tier: tests/test_gpu_half_table.py).

The bit contract of the half table -- a render from it equals the fp32 render of table.half().float() -- is a GPU statement.  What needs no device:
the rules of the Python surface (they fire before any device work), the model's routing, and how far a render of the widened table is from a
render of the full-precision one.  That last distance is a property of the field, measured here with the CPU oracle on the golden field and held to
the project's acceptance tolerance (RGB L-inf <= 1e-3)."""
import os
import re

import numpy as np
import pytest
import torch

from tests.common import load_golden, make_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def widened(table):
    """table.half().float(): what the half-table kernels compute with"""
    return torch.from_numpy(np.ascontiguousarray(table, np.float32)).half().float().numpy()


def test_entries_are_declared_and_the_rules_need_no_device():
    from avatarcraft_amd import _lib, nsr_ops
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    hdr = open(os.path.join(ROOT, "include", "avatarcraft_hip.h")).read()
    for name in ("ac_table_to_half", "ac_render_rays_h16", "ac_render_rays_warped_h16"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _lib.EXPORTS
    assert NeRFNetwork.render_table_dtype == "float"
    import inspect
    for fn in (nsr_ops.render_rays, nsr_ops.render_rays_long, nsr_ops.render_rays_pair):
        assert inspect.signature(fn).parameters["table_dtype"].default == "float"
    z = torch.zeros(4, 3)                                                         # CPU tensors, no field: anything past the rules would fail differently
    with pytest.raises(RuntimeError, match="train_extras"):
        nsr_ops.render_rays(None, z, z, 64, 64, train_extras=True, table_dtype="half")
    with pytest.raises(RuntimeError, match="opacity_only"):
        nsr_ops.render_rays(None, z, z, 64, 64, opacity_only=True, table_dtype="half")
    with pytest.raises(RuntimeError, match="table_dtype must be one of"):
        nsr_ops.render_rays(None, z, z, 64, 64, table_dtype="bfloat16")
    with pytest.raises(RuntimeError, match="long renderer reads the fp32 table"):
        nsr_ops.render_rays_long(None, z, z, 100, 64, table_dtype="half")
    with pytest.raises(RuntimeError, match="long renderer reads the fp32 table"):
        nsr_ops.render_rays_long(None, z, z, 64, 64, warp=object(), table_dtype="half")
    with pytest.raises(RuntimeError, match="pair launch"):
        nsr_ops.render_rays_pair(None, z, z, torch.zeros(8, 64), table_dtype="half")
    with pytest.raises(RuntimeError, match="CUDA tensor"):                        # the default goes on to today's argument checks
        nsr_ops.render_rays(None, z, z, 64, 64)


def test_render_of_the_widened_table_is_within_the_acceptance_bound(oracle):
    """oracle.render_rays on the golden field with its table and with table.half().float(): pixel L-inf <= 1e-3 on the golden rays.  The up-sampling's
    searchsorted indices that differ are counted and printed (a differing index moves one sample to the neighbouring bin; DESIGN section 5.9 records
    the figures)."""
    p = load_golden("nsr_params.npz")
    table = make_table(int(p["offsets"][-1]), seed=int(p["table_seed"]), offsets=p["offsets"], level_amp=p["level_amp"])
    t16 = widened(table)
    assert np.isfinite(t16).all() and (t16 != table).mean() > 0.9                # the rounding is real: nearly every entry moves
    mk = lambda t: oracle.Field(t, p["offsets"], p["W1"], p["b1"], p["W2"], p["b2"], p["Wc1"], p["Wc2"], p["Wc3"], float(p["per_level_scale"]))
    f32, f16 = mk(table), mk(t16)
    worst = 0.0
    for name in ("eval_64_64", "eval_32_32", "eval_edge"):
        g = load_golden(f"run_{name}.npz")
        T0, up = int(g["num_steps"]), int(g["upsample_steps"])
        a = oracle.render_rays(f32, g["rays_o"], g["rays_d"], T0, up, 1.6, float(p["inv_s"]), bg=g["bg"])
        b = oracle.render_rays(f16, g["rays_o"], g["rays_d"], T0, up, 1.6, float(p["inv_s"]), bg=g["bg"])
        d_img = float(np.abs(np.asarray(a["image"]) - np.asarray(b["image"])).max())
        d_ws = float(np.abs(np.asarray(a["weights_sum"]) - np.asarray(b["weights_sum"])).max())
        d_dep = float(np.abs(np.asarray(a["depth"]) - np.asarray(b["depth"])).max())
        n_ind = int((np.asarray(a["ss_inds"]) != np.asarray(b["ss_inds"])).sum()) if up else 0
        print(f"half table vs fp32 table, {name}: image L-inf {d_img:.3e}  weights_sum {d_ws:.3e}  depth {d_dep:.3e}  "
              f"searchsorted indices differing {n_ind} of {np.asarray(a['ss_inds']).size if up else 0}")
        worst = max(worst, d_img)
        assert d_img <= 1e-3, (name, d_img)
    assert worst > 0.0                                                           # (a table that survives the rounding unchanged would measure nothing)


class _Launched(Exception):
    pass


@pytest.fixture()
def routed(monkeypatch):
    """a default NeRFNetwork on the CPU whose render launches are recorded instead of made: (entry name, table_dtype it was given)"""
    from avatarcraft_amd import instant_nsr as M
    calls = []

    def recorder(name):
        def f(*a, **kw):
            calls.append((name, kw.get("table_dtype", "float")))
            raise _Launched(name)
        return f
    for name in ("render_rays", "render_rays_long", "render_rays_pair", "render_core", "sample_rays", "sample_rays_long"):
        monkeypatch.setattr(M.nsr_ops, name, recorder(name))
    monkeypatch.setattr(M.nsr_ops, "weight_norm_all", lambda layers: [None] * len(layers))
    monkeypatch.setattr(M.NeRFNetwork, "_field", lambda self: None)
    monkeypatch.setattr(M.NeRFNetwork, "_field_sdf_only", lambda self: None)
    torch.manual_seed(0)
    net = M.NeRFNetwork()
    ro = torch.zeros(1, 8, 3)
    rd = torch.zeros(1, 8, 3)
    rd[..., 2] = 1.0

    def run(num_steps=64, upsample_steps=64, **kw):
        del calls[:]
        try:
            net.run(ro, rd, num_steps, 1.6, upsample_steps, None, **kw)
        except _Launched:
            pass
        return list(calls)
    return net, run


def test_model_routes_half_to_no_grad_eval_renders_only(routed):
    net, run = routed
    net.eval()
    with torch.no_grad():
        assert run() == [("render_rays", "float")]                               # the default attribute: today's call
        net.render_table_dtype = "half"
        assert run() == [("render_rays", "half")]
        assert run(32, 32) == [("render_rays", "half")]
        with pytest.raises(NotImplementedError, match="fused renderer's window only"):
            net.run(torch.zeros(1, 8, 3), torch.ones(1, 8, 3), 128, 1.6, 128, None)
        with pytest.raises(NotImplementedError, match="fused renderer's window only"):
            net.run(torch.zeros(1, 8, 3), torch.ones(1, 8, 3), 100, 1.6, 64, None)
        net.train()
        assert run() == [("render_rays", "float")]                               # training mode reads the fp32 table, with or without gradients
        assert run(128, 128) == [("render_rays_long", "float")]                  # ... and keeps its long counts
        net.eval()
        net.render_table_dtype = "bfloat16"
        with pytest.raises(RuntimeError, match="render_table_dtype must be one of"):
            net.run(torch.zeros(1, 8, 3), torch.ones(1, 8, 3), 64, 1.6, 64, None)
        net.render_table_dtype = "half"
    # gradients wanted: every route of a differentiable render reads the fp32 table
    got = run()
    assert len(got) == 1 and got[0][1] == "float" and got[0][0] in ("render_core", "render_rays"), got
    net._manual_backward = True
    assert run() == [("render_rays", "float")]
    assert run(128, 128) == [("render_rays_long", "float")]
    for q in net.parameters():
        q.requires_grad_(False)
    assert run() == [("render_rays", "half")]                                    # nothing to differentiate: an inference render again
