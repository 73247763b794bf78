"""Training at the long renderer's counts, without a GPU: the routing predicates (NeRFNetwork.manual_backward_supported with and without counts,
stylize's call of it), the count envelope, and tests/golden/run_long_train.npz's own consistency."""
import os
import types

import numpy as np
import pytest

from tests.common import load_golden


def _stub(use_viewdirs, ok=True):
    return types.SimpleNamespace(fused_training="core" if ok else False, _fused_supported=lambda: True, use_viewdirs=use_viewdirs,
                                 encoder=types.SimpleNamespace(embeddings=types.SimpleNamespace(is_cuda=True)))


def test_manual_backward_supported_counts():
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    f = NeRFNetwork.manual_backward_supported
    for vd in (False, True):
        assert f(_stub(vd)) and f(_stub(vd), 64, 64) and f(_stub(vd), 128, 128) and f(_stub(vd), 96, 32) and f(_stub(vd), 256, 0)
        assert not f(_stub(vd, ok=False)) and not f(_stub(vd, ok=False), 128, 128)
    assert f(_stub(False), 100, 64) and f(_stub(False), 40, 16) and f(_stub(False), 2, 496)
    assert not f(_stub(True), 100, 64) and not f(_stub(True), 40, 16) and not f(_stub(True), 2, 496)     # view directions: T a multiple of 16
    assert f(_stub(True), 100) and f(_stub(True), upsample_steps=64)                                  # (both counts, or neither)


def test_sds_step_asks_with_counts_outside_the_window():
    from avatarcraft_amd.stylize import _manual_supported
    seen = []
    net = types.SimpleNamespace(manual_backward_supported=lambda *a: seen.append(a) or True)
    assert _manual_supported(net, 64, 64) and _manual_supported(net, 128, 128) and _manual_supported(net, 100, 64)
    assert seen == [(), (128, 128), (100, 64)]
    assert not _manual_supported(types.SimpleNamespace(), 128, 128)
    assert not _manual_supported(types.SimpleNamespace(manual_backward_supported=lambda: False), 64, 64)       # a zero-argument override


def test_count_envelope():
    from avatarcraft_amd import nsr_ops
    for ns, us in ((128, 128), (100, 64), (256, 0), (40, 16), (2, 496), (96, 32)):
        nsr_ops.check_long_counts(ns, us)
        assert not nsr_ops.in_short_window(ns, us)
    for ns, us in ((32, 32), (64, 64), (16, 112)):
        assert nsr_ops.in_short_window(ns, us)
    for ns, us, rule in ((100, 40, "multiple of 16"), (1, 16, "num_steps >= 2"), (400, 128, "<= 512")):
        with pytest.raises(RuntimeError, match=rule):
            nsr_ops.check_long_counts(ns, us)


def test_long_train_golden_is_consistent():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_long_train.npz")
    assert os.path.getsize(path) < 1 << 20
    g = load_golden("run_long_train.npz")
    p = load_golden("nsr_params.npz")
    n_rows = int(p["offsets"][-1])
    cases = sorted({k.split("/")[0] for k in g})
    assert cases == sorted(f"train_{a}_{b}" for a, b in ((128, 128), (100, 64), (256, 0), (40, 16)))
    for c in cases:
        ns, us = int(g[c + "/num_steps"]), int(g[c + "/upsample_steps"])
        assert c == f"train_{ns}_{us}"
        N = g[c + "/rays_o"].shape[0]
        assert N == 32 and g[c + "/noise"].shape == (N, ns) and g[c + "/G"].shape == (N, 3) and g[c + "/Gw"].shape == (N,)
        assert g[c + "/image"].shape == (N, 3) and g[c + "/weights_sum"].shape == (N,) and g[c + "/z_vals"].shape == (N, ns + us)
        assert (np.diff(g[c + "/z_vals"], axis=1) >= 0).all()
        ws = g[c + "/weights_sum"]
        assert np.isfinite(ws).all() and ws.min() >= 0.0 and ws.max() <= 1.0 + 1e-6
        assert 0.0 < float(g[c + "/gradient_error"]) < 1.0
        idx = g[c + "/emb_idx"]
        assert (np.diff(idx) > 0).all() and idx.min() >= 0 and idx.max() < n_rows
        eg = g[c + "/emb_grad"]
        assert eg.shape == (len(idx), 2) and np.abs(eg).max() <= float(g[c + "/emb_max"]) and (np.abs(eg).sum(1) > 0).all()
        names = {k[len(c) + 6:] for k in g if k.startswith(c + "/grad.")}
        assert {"deviation_net.variance", "sdf_net.0.weight_v", "sdf_net.1.bias", "color_net.0.weight_v", "color_net.2.weight_g"} <= names
        for k in names:
            assert np.isfinite(g[f"{c}/grad.{k}"]).all(), k
        assert np.abs(g[c + "/grad.color_net.0.weight_v"]).max() > 0 and abs(float(g[c + "/grad.deviation_net.variance"].reshape(-1)[0])) > 0
    # the same rays, background and upstream across the cases
    for k in ("rays_o", "rays_d", "bg", "G", "Gw"):
        for c in cases[1:]:
            assert np.array_equal(g[f"{cases[0]}/{k}"], g[f"{c}/{k}"]), k
