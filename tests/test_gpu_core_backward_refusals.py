"""-m gpu: a call that ac_render_core_backward refuses has queued nothing and written nothing.  The rows are the ones the library used to refuse only
after it had launched kernels (tests/golden/make_core_backward_rules.py: ROWS_AFTER_LAUNCH; their texts: tests/golden/core_backward_rules.json): each is
made on real, full-size device buffers -- so that even a wrongly accepted call would be a valid launch (the NULL weight pointer aside: that rule, like
every other, is also replayed where nothing can launch, tests/test_core_backward_rules_host.py) -- with the four gradient buffers and the scratch filled
with a byte pattern that must still be there afterwards; a valid call before the refused ones and one after them give the same bits.

Set-up: the synthetic field (with made-up view-direction weights for the rows that need a field with them), 16 rays at 16 + 16 samples -- the smallest
count with a coarse and an up-sampled tile -- and one training forward."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests.common import make_rays
from tests.gpu_common import device_field
from tests.test_core_backward_rules_host import generator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T0, UP = 16, 16, 16
PATTERN = 0xA5


def _setup():
    from avatarcraft_amd import _lib as L, nsr_ops
    from avatarcraft_amd.synthetic import load_field_params
    p = load_field_params()
    f, _ = device_field(p, device=DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    ro, rd = (t(a) for a in make_rays(4, 4, dist=1.7, f=6.4))
    rs = np.random.RandomState(3)
    out = nsr_ops.render_rays(f, ro, rd, T0, UP, 1.6, float(p["inv_s"]), noise=t(rs.uniform(0, 1, (N, T0))), extras=True, train_extras=True)
    T = T0 + UP
    e = dict(L=L, f=f, out=out, ro=ro, rd=rd, T=T, Wsh=t(rs.normal(0, 0.1, (64, 16))), sh_bias=t(rs.normal(0, 0.1, (N, 64))), near=t(np.full(N, 0.5)),
             far=t(np.full(N, 3.0)), up=[t(rs.normal(0, 1, s)) for s in ((N, 3), (N,), (N,), (N, 3))] + [t([0.01])],
             g_table=torch.empty_like(f.t["table"]), g_sdf=torch.empty(nsr_ops.SDF_PARAM_GRADS_LEN, device=DEV),
             g_col=torch.empty(nsr_ops.COLOR_PARAM_GRADS_LEN, device=DEV), g_invs=torch.empty(N, device=DEV),
             g_tiles=torch.empty((N * T // 16, 64), device=DEV))
    e["scratch"] = torch.empty(int(L.lib().ac_render_core_backward_scratch(C.byref(f.c), N, T)), dtype=torch.uint8, device=DEV)
    e["written"] = [e[k] for k in ("g_table", "g_sdf", "g_col", "g_invs", "scratch")]
    return e


def _call(e, c):
    """one ac_render_core_backward call on the set-up's buffers; c = the row's differences (the generator's CORE_ROWS) -> (status, message)"""
    L, out = e["L"], e["out"]
    c = dict(generator().CORE_VALID, **c)
    field = type(e["f"].c).from_buffer_copy(e["f"].c)
    field.offsets[16] -= c["offsets_cut"]
    if not c["W2"]:
        field.W2 = None
    if c["Wc1_sh"]:
        field.Wc1_sh = e["Wsh"].data_ptr()
    ns, us = c["counts"]
    assert N * (ns + us) <= N * e["T"]                                 # (the buffers are the valid call's: a smaller count fits them)
    op = L.ac_render_opts(N, ns, us, c["bound"], float(out.opts[0].inv_s), 1.0, c["fd_eps"], 0, None, e["near"].data_ptr() if c["near_m"] else None,
                          e["far"].data_ptr() if c["far_m"] else None, 0, 0, 0)
    feat7 = out["feat7"].data_ptr() if (ns + us) % 16 == 0 else None
    sv = L.ac_core_saved(*[out[k].data_ptr() for k in ("z_vals", "pts", "sdf", "sdf_out16", "gradient", "color")], out["eik_res"][1:].data_ptr(), feat7, None,
                         e["sh_bias"].data_ptr() if c["sh_bias"] else None)
    up = L.ac_core_upstream(*[g.data_ptr() for g in e["up"]], c["eik_group_rays"], c["eik_den_stride"])
    gr = L.ac_core_grads(e["g_table"].data_ptr(), e["g_sdf"].data_ptr(), e["g_col"].data_ptr(), e["g_invs"].data_ptr(), None, 0, 0,
                         e["g_tiles"].data_ptr() if c["g_sh_tiles"] else None)
    status = int(L.lib().ac_render_core_backward(C.byref(field), C.byref(op), e["ro"].data_ptr(), e["rd"].data_ptr(), None, C.byref(sv), C.byref(up),
                                                 C.byref(gr), e["scratch"].data_ptr(), e["scratch"].numel(), L.current_stream(torch.device(DEV))))
    return status, (L.lib().ac_last_error().decode() if status else "")


def _valid(e):
    for b in e["written"][:4]:
        b.zero_()
    assert _call(e, {}) == (0, "")
    torch.cuda.synchronize()
    return [b.clone() for b in e["written"][:4]]


def test_refused_calls_write_nothing_and_leave_no_state():
    G = generator()
    with open(G.FIXTURE) as f:
        rules = json.load(f)["rows"]
    e = _setup()
    before = _valid(e)
    assert all(float(b.abs().max()) > 0 for b in before)
    for b in e["written"]:
        b.view(torch.uint8).fill_(PATTERN)
    assert len(G.ROWS_AFTER_LAUNCH) == 11
    for row in G.ROWS_AFTER_LAUNCH:
        status, msg = _call(e, G.CORE_ROWS[row])
        torch.cuda.synchronize()
        assert [status, msg.split(": ", 1)[1]] == rules["render_core_backward." + row]["rule"], (row, status, msg)
        for name, b in zip(("g_table", "g_sdf_params", "g_color_params", "g_inv_s_per_ray", "scratch"), e["written"]):
            assert bool((b.view(torch.uint8) == PATTERN).all()), f"{row}: the refused call wrote to {name}"
    after = _valid(e)
    for name, a, b in zip(("g_table", "g_sdf_params", "g_color_params", "g_inv_s_per_ray"), before, after):
        assert torch.equal(a, b), name
