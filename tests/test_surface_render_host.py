"""CPU: the host side of the first-hit surface render (ac_render_rays_surface) -- the declaration and the ctypes mirrors of its two structs against the header
(a C program prints the layout), the refusals made before any device work, and the procedure itself as tests/surface_cases.py restates it around the CPU
oracle: its status histograms on the shared ray set and the invariants every stopped ray must meet."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import surface_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_entry_is_declared_and_bound():
    from avatarcraft_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "avatarcraft_hip.h")).read()
    assert re.search(r"\bint ac_render_rays_surface\s*\(", hdr) and "ac_render_rays_surface" in _lib.EXPORTS
    args, res = _lib._SIGS["ac_render_rays_surface"]
    assert len(args) == 8 and res is ctypes.c_int and args[1]._type_ is _lib.ac_surface_opts and args[6]._type_ is _lib.ac_surface_out


def test_struct_mirrors_match_the_header(tmp_path):
    from avatarcraft_amd import _lib
    names = {"ac_surface_opts": ["bound", "fd_eps", "level", "tol", "max_iters", "step_scale", "min_step", "guard"],
             "ac_surface_out": ["image", "weights_sum", "depth", "position", "normal_map", "sdf", "status", "iters"]}
    for s, fields in names.items():
        assert [f[0] for f in getattr(_lib, s)._fields_] == fields
    src = tmp_path / "layout.c"
    body = "".join('    printf("%zu' + " %zu" * len(f) + '\\n", sizeof(' + s + "), " + ", ".join(f"offsetof({s}, {k})" for k in f) + ");\n" for s, f in names.items())
    src.write_text('#include "avatarcraft_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True, timeout=60).stdout.strip().split("\n")
    for (s, fields), line, size in zip(names.items(), lines, (32, 64)):
        out = [int(x) for x in line.split()]
        assert out[0] == ctypes.sizeof(getattr(_lib, s)) == size, s
        assert out[1:] == [getattr(getattr(_lib, s), k).offset for k in fields], s
    assert _lib.ac_surface_opts.max_iters.size == 4


def test_cpu_tensors_and_bad_options_are_refused():
    from avatarcraft_amd import nsr_ops, drivers
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    o, d = (torch.from_numpy(a) for a in S.rays())
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        nsr_ops.render_rays_surface(None, o, d, S.BOUND, S.EPS)
    bad = [dict(max_iters=0), dict(max_iters=256), dict(max_iters=2.5), dict(tol=-1e-6), dict(tol=float("nan")), dict(step_scale=0.0), dict(step_scale=float("nan")),
           dict(min_step=0.0), dict(min_step=-1.0), dict(guard=0.5), dict(guard=-0.01), dict(guard=float("nan"))]
    for kw in bad:
        with pytest.raises(RuntimeError, match=next(iter(kw))):                # the option is named, and it is refused before the tensors are looked at
            nsr_ops.render_rays_surface(None, o, d, S.BOUND, S.EPS, **kw)
    for eps in (0.0, -0.005, float("nan"), 1e-60):
        with pytest.raises(RuntimeError, match="fd_eps"):
            nsr_ops.render_rays_surface(None, o, d, S.BOUND, eps)
    opts = nsr_ops.surface_opts(S.BOUND, S.EPS)
    assert (opts.level, opts.max_iters, opts.step_scale, opts.guard) == (0.0, 64, 1.0, 0.125) and opts.tol == F(1e-4) and opts.min_step == F(1e-3)
    assert nsr_ops.surface_opts(S.BOUND, S.EPS, max_iters=255, guard=0.0, tol=0.0).max_iters == 255
    # the model and the driver: a CPU model has no surface render, and says so before anything is computed
    torch.manual_seed(0)
    net = NeRFNetwork()
    with pytest.raises(RuntimeError, match="on the GPU"):
        net.render_surface(o[None], d[None], S.BOUND)
    assert "surface" in inspect.signature(drivers.render_canonical_360).parameters
    assert inspect.signature(drivers.render_canonical_360).parameters["surface"].default is False
    with pytest.raises(RuntimeError, match="on the GPU"):
        next(drivers.render_canonical_360(net, n_views=1, render_hw=(4, 4), with_head=False, device="cpu", surface=True))


@pytest.fixture(scope="module")
def traced(oracle, oracle_field):
    o, d = S.rays()
    assert o.shape == (588, 3) and d.shape == (588, 3) and o.dtype == F and d.dtype == F
    return {mi: S.restate(oracle, oracle_field, o, d, max_iters=mi) for mi in (64, 16, 1)}


def test_status_histograms_of_the_restatement(traced):
    for mi, r in traced.items():
        hist = np.bincount(r["status"], minlength=6).tolist()
        print(mi, hist, int(r["iters"].sum()))
        assert hist == S.HIST[mi], (mi, hist)
    assert all(c > 0 for c in S.HIST[16][:5])                                  # the condition: every status 0 - 4 is taken at max_iters = 16
    r = traced[64]
    assert int(r["iters"].astype(np.int64).sum()) == S.EVALS_64
    hit = r["status"] == 0
    assert hit.sum() >= 400 and np.abs(r["sdf"][hit]).max() <= 1.05e-4
    assert np.array_equal(r["sdf"][hit], r["trace"]["s"][hit])                 # the stencil's centre IS the tracer's last value (level 0)


def test_invariants_of_every_stopped_ray(traced):
    for mi, r in traced.items():
        st, tr = r["status"], r["trace"]
        t, near, far = tr["t"], tr["near"], tr["far"]
        assert (r["iters"] <= mi).all() and (r["iters"][far > near] >= 1).all() and (r["iters"][~(far > near)] == 0).all()
        assert (np.abs(tr["s"][st == 0]) <= F(S.TOL)).all()
        one = st == 1
        assert tr["bracketed"][one].all() and ((tr["t_lo"][one] <= t[one]) & (t[one] <= tr["t_hi"][one])).all()
        assert (tr["t_lo"][tr["bracketed"]] < tr["t_hi"][tr["bracketed"]]).all()
        two = st == 2
        assert ((t[two] >= far[two]) | (far[two] <= near[two])).all()
        assert (r["iters"][st == 3] == 1).all() and (t[st == 3] == near[st == 3]).all()
        assert not tr["bracketed"][st == 4].any() and (r["iters"][st == 4] == mi).all()
        shaded = np.isin(st, (0, 1, 3))
        assert np.array_equal(r["weights_sum"], shaded.astype(F)) and (r["depth"][~shaded] == 0).all() and (r["image"][~shaded] == 1).all()
        assert ((r["depth"][shaded] >= near[shaded]) & (r["depth"][shaded] <= far[shaded])).all()
        assert (np.abs(r["position"]) <= F(S.BOUND)).all() and all(np.isfinite(r[k]).all() for k in S.OUTPUTS)
