#!/usr/bin/env python3
"""Generate tests/golden/core_backward_rules.json: what ac_render_core_backward and the stand-alone training operators (ac_composite_*, ac_color_*,
ac_sdf_stencil_*, ac_sh_bias) answer to a call that breaks exactly one rule -- the status code and the ac_last_error() text behind its first ": " --
recorded WITHOUT a GPU at the commit before the whole-core backward checked all of its rules ahead of its first launch, so that the one check can be
compared with it row for row (tests/test_core_backward_rules_host.py replays the file against the built library).

    python tests/golden/make_core_backward_rules.py      (on a checkout whose avatarcraft_amd/ is exactly the parent commit's, built, on a machine
                                                          without a GPU: it refuses otherwise)

A row = one call, every argument valid (16 rays at 16 + 16 samples, host addresses that are never read) except the row's one violation.  The recorded
commit refused eleven of the whole-core rows only AFTER it had queued kernels (ROWS_AFTER_LAUNCH; without a device those launches fail and nothing runs),
four of them behind the colour backward's launch check (ROWS_BEHIND_LAUNCH_CHECK), which without a device reports the failed launch before the rule is
reached: for those four the parent's answer here is AC_ERR_LAUNCH.  Such a row stores that answer under "recorded" and, under "rule", the rule's own
answer -- AC_ERR_BAD_ARG and the text of the parent's source, the words the same rule is recorded with for a stand-alone entry where one has it.  Every
other row's "rule" is the parent's recorded answer itself.  The replay compares with "rule".
"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FIXTURE = os.path.join(HERE, "core_backward_rules.json")
AC_ERR_BAD_ARG, AC_ERR_LAUNCH = 1, 2
N, T0, UP = 16, 16, 16

_KEEP = (C.c_float * 64)()          # the one host address every non-NULL pointer gets: a refused call reads none of them
ADDR = C.addressof(_KEEP)

# ---- ac_render_core_backward: row -> what differs from the valid call
CORE_VALID = dict(counts=(T0, UP), fd_eps=0.005, bound=1.6, saved=True, rays_o=True, feat7=False, Wc1_sh=False, sh_bias=False, g_sh_tiles=False,
                  scratch_short=0, near_m=False, far_m=False, eik_group_rays=0, eik_den_stride=0, W2=True, offsets_cut=0)
CORE_ROWS = {
    "struct_null": dict(saved=False), "buffer_null": dict(rays_o=False), "fd_eps_0": dict(fd_eps=0.0),
    "feat7_T33": dict(counts=(17, 16), feat7=True), "sh_T33": dict(counts=(17, 16), Wc1_sh=True, sh_bias=True, g_sh_tiles=True),
    "scratch_short": dict(scratch_short=1), "counts_1_16": dict(counts=(1, 16)), "near_m_only": dict(near_m=True), "far_m_only": dict(far_m=True),
    "sh_without_bias": dict(Wc1_sh=True, g_sh_tiles=True), "bias_without_sh": dict(sh_bias=True), "sh_tiles_mismatch": dict(Wc1_sh=True, sh_bias=True),
    "eik_group_negative": dict(eik_group_rays=-1), "eik_group_no_stride": dict(eik_group_rays=4, eik_den_stride=0),
    "weight_null": dict(W2=False), "level_layout": dict(offsets_cut=8), "bound_0": dict(bound=0.0)}
# the rows the recorded commit refused after it had launched, in the order of its checks
ROWS_AFTER_LAUNCH = ["counts_1_16", "near_m_only", "far_m_only", "sh_without_bias", "bias_without_sh", "sh_tiles_mismatch", "weight_null",
                     "eik_group_negative", "eik_group_no_stride", "level_layout", "bound_0"]
# ... and those of them behind a launch check (weight_null is refused by the colour backward ahead of its own launch and check) -> the rule's text
ROWS_BEHIND_LAUNCH_CHECK = {"eik_group_negative": "eik_group_rays < 0 or eik_den_stride < 1", "eik_group_no_stride": "eik_group_rays < 0 or eik_den_stride < 1",
                            "level_layout": "level 15 is hashed with a non power-of-two size 524280; the fused renderer supports tables allocated by "
                                            "HashEncoder only (use ac_hash_encode_forward for arbitrary layouts)",
                            "bound_0": "eps and bound must be positive"}


def valid_field(L, c=None):
    c = c or {}
    p = np.load(os.path.join(HERE, "nsr_params.npz"))
    f = L.ac_field()
    for i, v in enumerate(p["offsets"]):
        f.offsets[i] = int(v)
    f.offsets[16] -= c.get("offsets_cut", 0)
    f.S, f.H = float(np.float32(np.log2(float(p["per_level_scale"])))), 16
    for k in ("table", "W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3"):
        setattr(f, k, ADDR)
    if not c.get("W2", True):
        f.W2 = None
    if c.get("Wc1_sh"):
        f.Wc1_sh = ADDR
    return f


def call_core(L, row):
    lib = L.lib()
    c = dict(CORE_VALID, **CORE_ROWS[row])
    ns, us = c["counts"]
    field = valid_field(L, c)
    op = L.ac_render_opts(N, ns, us, c["bound"], 1.0, 1.0, c["fd_eps"], 0, None, ADDR if c["near_m"] else None, ADDR if c["far_m"] else None, 0, 0, 0)
    sv = L.ac_core_saved(ADDR, ADDR, ADDR, ADDR, ADDR, ADDR, ADDR, ADDR if c["feat7"] else None, None, ADDR if c["sh_bias"] else None)
    up = L.ac_core_upstream(ADDR, ADDR, ADDR, ADDR, ADDR, c["eik_group_rays"], c["eik_den_stride"])
    gr = L.ac_core_grads(ADDR, ADDR, ADDR, ADDR, None, 0, 0, ADDR if c["g_sh_tiles"] else None)
    need = int(lib.ac_render_core_backward_scratch(C.byref(field), N, ns + us))
    return lib.ac_render_core_backward(C.byref(field), C.byref(op), ADDR if c["rays_o"] else None, ADDR, None, C.byref(sv) if c["saved"] else None,
                                       C.byref(up), C.byref(gr), ADDR, max(need - c["scratch_short"], 0), None)


# ---- the stand-alone operator entries: row -> the call (B = N * T samples)
B, T = N * (T0 + UP), T0 + UP


def _composite(L, fwd, counts=(T0, T), rays_o=ADDR, g_image=ADDR):
    head = [rays_o, ADDR, ADDR, ADDR, ADDR, ADDR, None, N, counts[0], counts[1], 1.6, 1.0, 1.0]
    if fwd:
        return L.lib().ac_composite_forward(*head, ADDR, ADDR, ADDR, ADDR, ADDR, ADDR, None)
    return L.lib().ac_composite_backward(*head, g_image, ADDR, ADDR, ADDR, ADDR, ADDR, ADDR, ADDR, None)


def _color_bwd(L, g_rgb=ADDR, short=0):
    f = valid_field(L)
    return L.lib().ac_color_backward(C.byref(f), ADDR, ADDR, ADDR, g_rgb, B, ADDR, ADDR, ADDR, ADDR, int(L.lib().ac_color_backward_scratch(B)) - short, None)


def _sdf_bwd(L, inputs, x=ADDR, g_x=ADDR, short=0):
    f = valid_field(L)
    need = int(L.lib().ac_sdf_stencil_backward_scratch(B)) - short
    if inputs:
        return L.lib().ac_sdf_stencil_backward_inputs(C.byref(f), x, ADDR, ADDR, B, 1.6, 0.005, ADDR, ADDR, g_x, ADDR, need, None)
    return L.lib().ac_sdf_stencil_backward(C.byref(f), x, ADDR, ADDR, B, 1.6, 0.005, ADDR, ADDR, ADDR, need, None)


OP_ROWS = {
    "composite_forward.counts_1_17": lambda L: _composite(L, True, counts=(1, 17)),
    "composite_forward.buffer_null": lambda L: _composite(L, True, rays_o=None),
    "composite_backward.counts_1_17": lambda L: _composite(L, False, counts=(1, 17)),
    "composite_backward.buffer_null": lambda L: _composite(L, False, g_image=None),
    "color_forward.buffer_null": lambda L: L.lib().ac_color_forward(C.byref(valid_field(L)), ADDR, ADDR, ADDR, B, None, None),
    "color_forward.weight_null": lambda L: L.lib().ac_color_forward(C.byref(valid_field(L, dict(W2=False))), ADDR, ADDR, ADDR, B, ADDR, None),
    "color_backward.buffer_null": lambda L: _color_bwd(L, g_rgb=None),
    "color_backward.scratch_short": lambda L: _color_bwd(L, short=1),
    "sdf_stencil_forward.eps_0": lambda L: L.lib().ac_sdf_stencil_forward(C.byref(valid_field(L)), ADDR, B, 1.6, 0.0, ADDR, ADDR, None),
    "sdf_stencil_forward.level_layout": lambda L: L.lib().ac_sdf_stencil_forward(C.byref(valid_field(L, dict(offsets_cut=8))), ADDR, B, 1.6, 0.005, ADDR, ADDR, None),
    "sdf_stencil_backward.buffer_null": lambda L: _sdf_bwd(L, False, x=None),
    "sdf_stencil_backward.scratch_short": lambda L: _sdf_bwd(L, False, short=1),
    "sdf_stencil_backward_inputs.g_x_null": lambda L: _sdf_bwd(L, True, g_x=None),
    "sdf_stencil_backward_inputs.scratch_short": lambda L: _sdf_bwd(L, True, short=1),
    "sh_bias.no_view_directions": lambda L: L.lib().ac_sh_bias(C.byref(valid_field(L)), ADDR, N, ADDR, None, None),
    "sh_bias.buffer_null": lambda L: L.lib().ac_sh_bias(C.byref(valid_field(L, dict(Wc1_sh=True))), None, N, ADDR, None, None)}
ROWS = ["render_core_backward." + r for r in CORE_ROWS] + list(OP_ROWS)


def call(L, row):
    """-> [status, the error text behind its first ": "] of one row"""
    entry, name = row.split(".", 1)
    status = int(call_core(L, name) if entry == "render_core_backward" else OP_ROWS[row](L))
    msg = L.lib().ac_last_error().decode() if status else ""
    return [status, msg.split(": ", 1)[1] if ": " in msg else msg]


def main():
    git = lambda *a: subprocess.run(("git",) + a, cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    if git("status", "--porcelain", "--", "avatarcraft_amd"):
        sys.exit("avatarcraft_amd/ differs from HEAD: the fixture is recorded from a committed parent, never from a working tree")
    if os.path.exists("/dev/kfd"):
        sys.exit("this machine has a GPU: a rule the parent checks late would be reached after launches on addresses that are not device memory; record without one")
    from avatarcraft_amd import _lib as L
    rows = {}
    for row in ROWS:
        got = call(L, row)
        rule = ROWS_BEHIND_LAUNCH_CHECK.get(row.split(".", 1)[1]) if row.startswith("render_core_backward.") else None
        if rule is None:
            assert got[0] == AC_ERR_BAD_ARG, (row, got)
            rows[row] = {"rule": got}
        else:                                                          # see the module docstring
            assert got[0] == AC_ERR_LAUNCH and got[1].startswith("no ROCm-capable device") or got == [AC_ERR_BAD_ARG, rule], (row, got)
            rows[row] = {"rule": [AC_ERR_BAD_ARG, rule], "recorded": got}
    doc = {"header": {"parent_commit": git("rev-parse", "HEAD"), "generator": "tests/golden/make_core_backward_rules.py", "n_rays": N,
                      "counts": [T0, UP]}, "rows": rows}
    with open(FIXTURE, "w") as f:                                      # one row per line: a changed answer shows as a changed line
        f.write('{"header": %s,\n "rows": {\n  %s}}\n' % (json.dumps(doc["header"]), ",\n  ".join('"%s": %s' % (k, json.dumps(v)) for k, v in rows.items())))
    assert json.load(open(FIXTURE)) == doc
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes:", len(rows), "rows,", sum("recorded" in r for r in rows.values()), "behind a launch check")


if __name__ == "__main__":
    main()
