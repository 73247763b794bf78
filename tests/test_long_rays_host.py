"""CPU tier of the long renderer (render_rays_long / sample_rays_long): argument rules checked before any device work and the fixture the GPU
tier reads (tests/golden/run_long.npz).  test_linspace_tables_any_length pins a property the long renderer relies on (linspace_tables already
had it before the long renderer existed, so it is not a test of new behaviour)."""
import numpy as np
import pytest
import torch

from tests.common import load_golden

CASES = ["eval_128_128", "eval_100_64", "eval_256_0", "eval_96_32", "eval_40_16", "eval_16_496", "train_96_32"]


@pytest.mark.parametrize("n", [2, 100, 256, 512])
def test_linspace_tables_any_length(n):
    from avatarcraft_amd import nsr_ops
    lin_z, lin_u = nsr_ops.linspace_tables(n, "cpu")
    assert lin_z.shape == (n,)
    assert torch.equal(lin_z.view(torch.int32), torch.linspace(0.0, 1.0, n, dtype=torch.float32).view(torch.int32))
    assert torch.equal(lin_u, torch.linspace(0.5 / 16, 1 - 0.5 / 16, 16, dtype=torch.float32))


class _NoField:
    """a field that must never be touched: the checks come first"""
    def __getattr__(self, name):
        raise AssertionError(f"field.{name} used before the arguments were checked")


@pytest.mark.parametrize("fn", ["render_rays_long", "sample_rays_long"])
@pytest.mark.parametrize("T0,up,rule", [(64, 40, "multiple of 16"), (1, 16, "num_steps >= 2"), (0, 0, "num_steps >= 2"), (64, -16, "upsample_steps >= 0"),
                                        (400, 128, "<= 512"), (513, 0, "<= 512")])
def test_counts_outside_envelope_rejected(fn, T0, up, rule):
    from avatarcraft_amd import nsr_ops
    ro = torch.zeros(4, 3, dtype=torch.float32)
    with pytest.raises(RuntimeError, match=rule):
        getattr(nsr_ops, fn)(_NoField(), ro, ro, T0, up, 1.6)


@pytest.mark.parametrize("fn", ["render_rays_long", "sample_rays_long"])
@pytest.mark.parametrize("T0,up", [(128, 128), (100, 64), (2, 0), (512, 0)])
def test_cpu_tensors_rejected(fn, T0, up):
    from avatarcraft_amd import nsr_ops
    ro = torch.zeros(4, 3, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        getattr(nsr_ops, fn)(_NoField(), ro, ro, T0, up, 1.6)


def test_long_counts_leave_the_fused_window():
    from avatarcraft_amd import nsr_ops
    for T0, up in ((16, 0), (32, 32), (64, 64), (16, 112)):
        assert nsr_ops.in_short_window(T0, up)
    for T0, up in ((128, 128), (100, 64), (96, 32), (60, 64), (64, 80), (256, 0)):
        assert not nsr_ops.in_short_window(T0, up)


def test_run_long_fixture_has_every_key():
    gd = load_golden("run_long.npz")
    for name in CASES:
        T0, up = (int(v) for v in name.split("_")[1:])
        g = lambda k: gd[f"{name}/{k}"]
        N = g("rays_o").shape[0]
        assert N == 32 and int(g("num_steps")) == T0 and int(g("upsample_steps")) == up
        for k, shape in (("rays_d", (N, 3)), ("bg", (N, 3)), ("image", (N, 3)), ("weights_sum", (N,)), ("depth", (N,)), ("normal_map", (N, 3)),
                         ("z_vals", (N, T0 + up)), ("ss_inds", (N, up // 16, 16)), ("sort_index", (N, max(up // 16, 1), T0 + up))):
            assert g(k).shape == shape, (name, k)
        assert g("oracle_ss_flips").shape[1] == 3
        assert np.isfinite(g("image")).all() and np.isfinite(g("gradient_error"))
    tr = lambda k: gd[f"train_96_32/{k}"]
    assert tr("noise").shape == (32, 96)
    assert tr("emb_grad").shape == (tr("emb_idx").shape[0], 2) and float(tr("emb_max")) > 0
    for k in ("sdf_net.0.weight_g", "sdf_net.0.weight_v", "sdf_net.0.bias", "sdf_net.1.weight_v", "color_net.0.weight_v", "color_net.2.weight_g",
              "deviation_net.variance"):
        assert f"train_96_32/grad.{k}" in gd, k
