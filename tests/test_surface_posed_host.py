"""CPU: the host side of the posed first-hit surface render (ac_render_rays_surface_warped) -- the declaration and the ctypes mirror of its new struct against the
header (a C program prints the layout), the refusals made before any device work (Python's and the C entry's own), and the procedure itself as
tests/surface_posed_cases.py restates it around the CPU oracle: its status histograms on the shared case and the invariants every stopped ray must meet.
Measured here (golden field, make_body(), the 400 camera rays, the defaults): 13.0 searches and 2.8 SDF evaluations per ray; 74 shaded rays of which 34 are cuts
at the mask boundary (status 6) -- the golden field's body is wider than the mask of make_body()."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import surface_posed_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAME = "ac_render_rays_surface_warped"


def test_entry_is_declared_and_bound():
    from avatarcraft_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "avatarcraft_hip.h")).read()
    assert re.search(r"\bint %s\s*\(" % NAME, hdr) and re.search(r"\bsize_t %s_scratch\s*\(" % NAME, hdr)
    assert NAME in _lib.EXPORTS and NAME + "_scratch" in _lib.EXPORTS
    args, res = _lib._SIGS[NAME]
    assert len(args) == 13 and res is ctypes.c_int and args[2] is ctypes.c_float
    assert args[1]._type_ is _lib.ac_surface_opts and args[7]._type_ is _lib.ac_warp_mesh and args[10]._type_ is _lib.ac_surface_out
    assert args[11]._type_ is _lib.ac_surface_warped_out
    assert _lib._SIGS[NAME + "_scratch"] == ([ctypes.c_uint32], ctypes.c_size_t)
    assert _lib.lib().ac_version() == 10


def test_struct_mirror_matches_the_header(tmp_path):
    from avatarcraft_amd import _lib
    fields = ["canonical", "normal_can", "face_id"]
    assert [f[0] for f in _lib.ac_surface_warped_out._fields_] == fields
    src = tmp_path / "layout.c"
    s = "ac_surface_warped_out"
    src.write_text('#include "avatarcraft_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n    printf("%zu %zu %zu %zu\\n", sizeof(' + s + "), "
                   + ", ".join(f"offsetof({s}, {k})" for k in fields) + ");\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True, timeout=60).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.ac_surface_warped_out) == 24
    assert out[1:] == [getattr(_lib.ac_surface_warped_out, k).offset for k in fields]


def test_cpu_tensors_and_bad_options_are_refused():
    from avatarcraft_amd import nsr_ops, drivers
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    o, d = (torch.from_numpy(a) for a in P.rays())
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        nsr_ops.render_rays_surface_warped(None, o, d, P.BOUND, None)
    bad = [dict(max_iters=0), dict(max_iters=256), dict(max_iters=2.5), dict(tol=-1e-6), dict(tol=float("nan")), dict(step_scale=0.0), dict(min_step=0.0),
           dict(guard=0.5), dict(guard=float("nan")), dict(w_tol=-1e-6), dict(w_tol=float("nan")), dict(w_tol="wide")]
    for kw in bad:
        with pytest.raises(RuntimeError, match="render_rays_surface_warped: .*" + next(iter(kw))):      # named, and refused before the tensors are looked at
            nsr_ops.render_rays_surface_warped(None, o, d, P.BOUND, None, **kw)
    with pytest.raises(RuntimeError, match="fd_eps"):
        nsr_ops.render_rays_surface_warped(None, o, d, P.BOUND, None, 0.0)
    opts, w_tol = nsr_ops.surface_warped_opts(P.BOUND, P.EPS)
    assert (opts.level, opts.max_iters, opts.step_scale, opts.guard) == (0.0, 64, 1.0, 0.125) and opts.tol == F(1e-4) and w_tol == 1e-4
    assert nsr_ops.surface_warped_opts(P.BOUND, P.EPS, w_tol=0)[1] == 0.0
    torch.manual_seed(0)
    net = NeRFNetwork()
    v, f, T = P.body()
    with pytest.raises(RuntimeError, match="on the GPU"):
        net.render_surface_posed(o[None], d[None], P.BOUND, v, f, T)
    sig = inspect.signature(drivers.render_animation).parameters
    assert "surface" in sig and sig["surface"].default is False
    assert list(inspect.signature(NeRFNetwork.render_surface_posed).parameters)[:9] == ["self", "rays_o", "rays_d", "bound", "verts", "faces", "Ts", "bg_color",
                                                                                          "max_ray_batch"]


def test_the_entry_refuses_before_any_launch():
    """AC_ERR_BAD_ARG (1) comes back before the field is looked at or anything is launched: this runs without a device"""
    from avatarcraft_amd import _lib as L
    lib = L.lib()
    N = 16
    buf = (ctypes.c_float * (3 * N))()
    st = (ctypes.c_uint8 * N)()
    dbl = (ctypes.c_double * 16)()
    idx = (ctypes.c_int32 * 3)()
    adr = lambda a: ctypes.cast(a, ctypes.c_void_p).value
    field = L.ac_field()
    out = L.ac_surface_out(None, None, None, None, None, None, adr(st), None)
    good = lambda: L.ac_surface_opts(1.6, 0.005, 0.0, 1e-4, 64, 1.0, 1e-3, 0.125)
    mesh = lambda **kw: L.ac_warp_mesh(**{**dict(verts=adr(buf), faces=adr(idx), T=adr(dbl), V=1, F=1, threshold=0.05, geo_threshold=0.05, use_mesh_guide=0, accel=None,
                                                  seed_faces=None, seed_stride=0), **kw})
    need = lib.ac_render_rays_surface_warped_scratch(N)
    assert need >= 90 * N and lib.ac_render_rays_surface_warped_scratch(4096) >= 90 * 4096 and lib.ac_render_rays_surface_warped_scratch(0) == 0
    scratch = (ctypes.c_uint8 * need)()

    def call(opts=None, w_tol=1e-4, m=None, n=N, scr=adr(scratch), nbytes=need, o=out, rays=adr(buf), null_mesh=False):
        opts = opts or good()
        m = m or mesh()
        return lib.ac_render_rays_surface_warped(ctypes.byref(field), ctypes.byref(opts), w_tol, rays, rays, n, None, None if null_mesh else ctypes.byref(m), scr, nbytes,
                                                 ctypes.byref(o), None, None)

    def refused(match, **kw):
        assert call(**kw) == 1, kw
        assert re.search(match, lib.ac_last_error().decode()), (match, lib.ac_last_error())

    for name, v in (("max_iters", 0), ("max_iters", 256), ("tol", -1.0), ("tol", float("nan")), ("fd_eps", 0.0), ("step_scale", 0.0), ("min_step", 0.0), ("bound", 0.0),
                    ("guard", 0.5), ("guard", -0.1)):
        o = good()
        setattr(o, name, v)
        refused(name, opts=o)
    refused("w_tol", w_tol=-1e-6)
    refused("w_tol", w_tol=float("nan"))
    refused("mesh", null_mesh=True)
    for k in ("verts", "faces", "T"):
        refused("mesh", m=mesh(**{k: None}))
    refused("faces", m=mesh(F=0))
    refused("scratch", nbytes=need - 1)
    refused("scratch", scr=None)
    refused("rays", rays=None)
    refused("status", o=L.ac_surface_out())
    assert call(n=0) == 0                                                        # nothing to do: nothing launched
    assert call(n=0, w_tol=-1.0) == 1                                            # ... but a bad option is refused whatever N is


@pytest.fixture(scope="module")
def traced(oracle, oracle_field):
    o, d = P.rays()
    v, f, T = P.body()
    assert o.shape == (415, 3) and d.dtype == F and v.shape == (3202, 3) and f.shape == (6400, 3)
    return {mi: P.restate_posed(oracle, oracle_field, o, d, v, f, T, max_iters=mi) for mi in (64, 16, 1)}


def test_status_histograms_of_the_restatement(traced):
    n = P.N_CAMERA
    for mi, r in traced.items():
        cam, every = np.bincount(r["status"][:n], minlength=7).tolist(), np.bincount(r["status"], minlength=7).tolist()
        print(mi, cam, every, r["trace"]["searches"], r["trace"]["sdf_evals"])
        assert cam == P.HIST_CAMERA[mi] and every == P.HIST_ALL[mi], (mi, cam, every)
    # the conditions on the case
    assert all(P.HIST_CAMERA[64][s] >= 20 for s in (0, 2, 6))
    assert P.HIST_CAMERA[16][1] > 0 and P.HIST_CAMERA[16][4] > 0
    r = traced[64]
    assert r["status"][n + 12:n + 14].tolist() == [3, 3]                          # the two rays that start inside the posed body
    # the NaN origin: near and far are NaN, `far > near` is false -> status 2 without a search (in numpy's slab test as in the device's); no ray over a finite
    # field can reach status 5 -- the NaN-table test below does
    assert r["status"][n + 14] == 2 and r["iters"][n + 14] == 0
    assert int(r["iters"][:n].astype(np.int64).sum()) == P.SEARCHES_64
    cam_only = {k: v for k, v in r.items() if k != "trace"}
    assert int(cam_only["weights_sum"][:n].sum()) == 74


def test_a_nan_table_gives_status_5(oracle, golden_params):
    from tests.common import make_table
    p = golden_params
    table = np.full_like(make_table(int(p["offsets"][-1]), seed=int(p["table_seed"]), offsets=p["offsets"], level_amp=p["level_amp"]), np.nan)
    nf = oracle.Field(table, p["offsets"], p["W1"], p["b1"], p["W2"], p["b2"], p["Wc1"], p["Wc2"], p["Wc3"], float(p["per_level_scale"]))
    o, d = P.rays()
    v, f, T = P.body()
    r = P.restate_posed(oracle, nf, o, d, v, f, T)
    hist = np.bincount(r["status"], minlength=7).tolist()
    print(hist)
    assert hist[5] >= 60 and hist[0] == hist[1] == hist[3] == hist[6] == 0 and hist[2] + hist[5] == 415      # every ray that reaches the mask stops there
    assert (r["weights_sum"] == 0).all() and (r["image"] == 1).all() and (r["face_id"] == -1).all()


def test_invariants_of_every_stopped_ray(traced):
    for mi, r in traced.items():
        st, tr = r["status"], r["trace"]
        near, far = tr["near"], tr["far"]
        with np.errstate(invalid="ignore"):
            live = far > near
        assert (r["iters"] <= mi).all() and (r["iters"][live] >= 1).all() and (r["iters"][~live] == 0).all()
        shaded = np.isin(st, P.SHADED)
        assert tr["mask_s"][shaded].all()                                         # every shaded point is unmasked
        assert (np.abs(r["sdf"][st == 0]) <= F(P.TOL)).all()                      # a hit is unmasked and on the level set
        six = st == 6
        assert ((tr["t_hi"][six] - tr["t_lo"][six]) <= F(P.W_TOL)).all() and (tr["lo_masked"][six] | (tr["s_lo"][six] > 0)).all() and (tr["s_hi"][six] < 0).all()
        assert (r["depth"][six] == tr["t_hi"][six]).all() and (r["depth"][st == 1] == tr["t_hi"][st == 1]).all()
        assert (tr["t_lo"][tr["bracketed"]] < tr["t_hi"][tr["bracketed"]]).all()
        assert (r["iters"][st == 3] == 1).all() and not tr["bracketed"][st == 4].any() and (r["iters"][st == 4] == mi).all()
        assert (r["depth"][shaded] <= far[shaded]).all() and (r["depth"][shaded] >= near[shaded]).all()
        assert np.array_equal(r["weights_sum"], shaded.astype(F)) and (r["image"][~shaded] == 1).all() and (r["face_id"][~shaded] == -1).all()
        for k in ("depth", "position", "normal_map", "sdf", "canonical", "normal_can"):
            assert (r[k][~shaded] == 0).all() and np.isfinite(r[k]).all(), k
        assert (r["face_id"][shaded] >= 0).all() and (r["face_id"][shaded] < 6400).all()
        assert np.abs(np.linalg.norm(r["normal_map"][shaded].astype(np.float64), axis=1) - 1.0).max() < 1e-6
