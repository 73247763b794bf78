#!/usr/bin/env python3
"""Generate tests/golden/render_entry_rules.json: what each of the ten C entries of the ray renderers answers to one broken argument -- the status code and
the ac_last_error() text -- recorded WITHOUT a GPU at the commit before their host code became one driver, so that the shared check can be compared with
it cell for cell (tests/test_render_entry_rules_host.py replays the file against the built library).

    python tests/golden/make_render_entry_rules.py       (on a checkout whose avatarcraft_amd/ is exactly the parent commit's, built, on a machine
                                                          without a GPU: it refuses otherwise)

A cell = one entry x one row of ROWS: every argument valid (16 rays at 32 + 32, host addresses that are never read) except the row's one violation.
Every check of an entry runs before any device work, so a refused call touches no buffer.  A call the parent ACCEPTS with n_rays > 0 would launch:
such a cell is not recorded -- its entry is only named under the row's "launches" (without a GPU the launch fails and nothing runs; the generator refuses
to run where one exists) -- and is never replayed.  Each row is recorded a second time with n_rays = 0 ("n0": nothing can launch, every cell is kept).
"scratch" holds ac_render_rays_warped_scratch(N, T, offs): the size and the six documented offsets.

"amended" lists the cells whose answer the shared check changes on purpose, with the parent's answer next to the new one: an entry of the short window
called with n_rays <= 0 and an invalid precision, skip_masked, opacity_only or near_m / far_m pairing used to return AC_OK (its early return came before
those rules); it is now refused with that rule, as the long entries always did.  "rows" itself stays the parent's recording.
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

FIXTURE = os.path.join(HERE, "render_entry_rules.json")
AC_ERR_BAD_ARG = 1

# entry -> (long window, posed, pair, half table, sampling only)
ENTRIES = {"ac_render_rays": (0, 0, 0, 0, 0), "ac_render_rays_h16": (0, 0, 0, 1, 0), "ac_render_rays_pair": (0, 0, 1, 0, 0),
           "ac_sample_rays": (0, 0, 0, 0, 1), "ac_render_rays_warped": (0, 1, 0, 0, 0), "ac_render_rays_warped_h16": (0, 1, 0, 1, 0),
           "ac_render_rays_long": (1, 0, 0, 0, 0), "ac_render_rays_long_pair": (1, 0, 1, 0, 0), "ac_sample_rays_long": (1, 0, 0, 0, 1),
           "ac_render_rays_long_warped": (1, 1, 0, 0, 0)}
MANDATORY = ("image", "weights_sum", "depth", "normal_map", "eik")
COUNTS = [(0, 16), (1, 16), (2, 16), (20, 16), (32, 40), (64, 64), (80, 48), (64, 80), (400, 128), (384, 128)]
VALID = dict(n_rays=16, counts=(32, 32), fd_eps=0.005, precision=0, skip_masked=0, opacity_only=0, near_m=False, far_m=False, perturb=0,
             rays_o=True, lin_u=True, out=True, opts=True, out_null=(), out_set=(), half_table=True, mesh="full", scratch_short=0)
ROWS = {"valid": {}}
ROWS.update({"counts_%d_%d" % c: dict(counts=c) for c in COUNTS})
ROWS.update({"fd_eps_0": dict(fd_eps=0.0), "precision_7": dict(precision=7), "skip_masked_1": dict(skip_masked=1), "skip_masked_2": dict(skip_masked=2),
             "opacity_only_1": dict(opacity_only=1), "opacity_only_2": dict(opacity_only=2), "near_m_only": dict(near_m=True), "far_m_only": dict(far_m=True),
             "rays_o_null": dict(rays_o=False), "lin_u_null": dict(lin_u=False), "perturb_no_noise": dict(perturb=1)})
ROWS.update({"out_%s_null" % k: dict(out_null=(k,)) for k in MANDATORY})
ROWS.update({"feat7_T164": dict(counts=(100, 64), out_set=("feat7",)), "feat7_T128": dict(counts=(64, 64), out_set=("feat7",)),
             "sdf_out16_set": dict(out_set=("sdf_out16",)), "half_table_null": dict(half_table=False), "mesh_null": dict(mesh=None),
             "mesh_no_faces": dict(mesh="no_faces"), "scratch_short": dict(scratch_short=1), "out_null": dict(out=False), "opts_null": dict(opts=False),
             "pair_limit": dict(n_rays=(1 << 29) + 1)})
N0_ROWS = [r for r in ROWS if r != "pair_limit"]                       # (that row's violation is its ray count)
SCRATCH_SHAPES = [(0, 0), (1, 16), (16, 164), (4096, 128), (65536, 512), (1000, 100)]
SHORT = [e for e, k in ENTRIES.items() if not k[0]]
AMENDED_ROWS = {"precision_7": "precision 7 unknown (0 = exact, 1 = fast)", "skip_masked_2": "skip_masked must be 0 or 1",
                "opacity_only_2": "opacity_only must be 0 or 1", "near_m_only": "near_m and far_m go together", "far_m_only": "near_m and far_m go together"}


def amended():
    """[{"row", "entry", "parent": [status, message], "now": [status, message]}]: see the module docstring"""
    res = []
    for row, text in AMENDED_ROWS.items():
        for e in SHORT:
            if row == "opacity_only_2" and ENTRIES[e][3]:
                continue                                               # (the half table's own rule already refuses any opacity_only before the early return)
            res.append({"row": row, "entry": e, "parent": [0, ""], "now": [AC_ERR_BAD_ARG, "%s: %s" % (e[3:], text)]})
    return res


_KEEP = (C.c_float * 64)()          # the one host address every non-NULL pointer gets: a refused call reads none of them
ADDR = C.addressof(_KEEP)


def valid_field(L):
    p = np.load(os.path.join(HERE, "nsr_params.npz"))
    f = L.ac_field()
    for i, v in enumerate(p["offsets"]):
        f.offsets[i] = int(v)
    f.S, f.H = float(np.float32(np.log2(float(p["per_level_scale"])))), 16
    for k in ("table", "W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3"):
        setattr(f, k, ADDR)
    return f


def call(L, entry, row, n_rays=None):
    """-> (status, message) of one cell"""
    lib = L.lib()
    c = dict(VALID, **ROWS[row])
    if n_rays is not None:
        c["n_rays"] = n_rays
    _, posed, _, h16, sampling = ENTRIES[entry]
    ns, us = c["counts"]
    op = L.ac_render_opts(c["n_rays"], ns, us, 1.6, 1.0, 1.0, c["fd_eps"], c["perturb"], None, ADDR if c["near_m"] else None, ADDR if c["far_m"] else None,
                          c["precision"], c["skip_masked"], c["opacity_only"])
    out = L.ac_render_out()
    for k in MANDATORY + tuple(c["out_set"]):
        setattr(out, k, None if k in c["out_null"] else ADDR)
    field = valid_field(L)
    a = [C.byref(field)]
    if h16:
        a.append(ADDR if c["half_table"] else None)
    a += [C.byref(op) if c["opts"] else None, ADDR if c["rays_o"] else None, ADDR]
    if not sampling:
        a.append(None)                                                 # bg
    a += [None, ADDR, ADDR if c["lin_u"] else None]                    # noise, lin_z, lin_u
    if posed:
        mesh = L.ac_warp_mesh(ADDR, ADDR, ADDR, 4, 0 if c["mesh"] == "no_faces" else 2, 0.05, 0.05, 0, None, None, 0)
        need = int(lib.ac_render_rays_warped_scratch(c["n_rays"], ns + us, None))
        a += [C.byref(mesh) if c["mesh"] else None, ADDR, max(need - c["scratch_short"], 0)]
    a.append((ADDR if c["out"] else None) if sampling else (C.byref(out) if c["out"] else None))
    status = int(getattr(lib, entry)(*a, None))
    return status, (lib.ac_last_error().decode() if status else "")


def record_all(L):
    rows = {}
    for row in ROWS:
        r = rows[row] = {"n16": {}, "launches": []}
        for e in ENTRIES:
            status, msg = call(L, e, row)
            if status == AC_ERR_BAD_ARG:
                r["n16"][e] = [status, msg]
            else:                                                      # accepted: not recorded (see the module docstring)
                r["launches"].append(e)
        if row in N0_ROWS:
            r["n0"] = {e: list(call(L, e, row, n_rays=0)) for e in ENTRIES}
    assert rows["valid"]["launches"] == list(ENTRIES), "the base case must be valid for every entry: " + json.dumps(rows["valid"]["n16"])
    return rows


def record_scratch(L):
    res = []
    for n, t in SCRATCH_SHAPES:
        offs = (C.c_size_t * 6)()
        res.append([n, t, int(L.lib().ac_render_rays_warped_scratch(n, t, offs)), [int(v) for v in offs]])
    return res


def main():
    git = lambda *a: subprocess.run(("git",) + a, cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    if git("status", "--porcelain", "--", "avatarcraft_amd"):
        sys.exit("avatarcraft_amd/ differs from HEAD: the fixture is recorded from a committed parent, never from a working tree")
    if os.path.exists("/dev/kfd"):
        sys.exit("this machine has a GPU: a case the parent accepts would launch on addresses that are not device memory; record without one")
    from avatarcraft_amd import _lib as L
    rows = record_all(L)
    am = amended()
    for c in am:
        assert rows[c["row"]]["n0"][c["entry"]] == c["parent"], c      # an amended cell is one the parent's early return hid
    doc = {"header": {"parent_commit": git("rev-parse", "HEAD"), "generator": "tests/golden/make_render_entry_rules.py", "n_rays": VALID["n_rays"],
                      "counts": list(VALID["counts"])}, "entries": list(ENTRIES), "rows": rows, "scratch": record_scratch(L), "amended": am}
    with open(FIXTURE, "w") as f:                                      # one row and tier per line: a changed answer shows as a changed line
        f.write('{"header": %s,\n "entries": %s,\n "rows": {' % (json.dumps(doc["header"]), json.dumps(doc["entries"])))
        f.write(",".join('\n  "%s": {%s}' % (name, ",\n    ".join('"%s": %s' % (k, json.dumps(v)) for k, v in r.items())) for name, r in rows.items()))
        f.write('},\n "scratch": %s,\n "amended": [\n  %s]}\n' % (json.dumps(doc["scratch"]), ",\n  ".join(json.dumps(c) for c in am)))
    assert json.load(open(FIXTURE)) == json.loads(json.dumps(doc))
    n16 = sum(len(r["n16"]) for r in rows.values())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes:", n16, "refused cells at 16 rays,", sum(len(r["launches"]) for r in rows.values()),
          "accepted (not recorded),", sum(len(r.get("n0", ())) for r in rows.values()), "cells at 0 rays,", len(am), "amended")


if __name__ == "__main__":
    main()
