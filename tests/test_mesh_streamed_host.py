"""CPU tier of the streamed mesh export (ac_marching_cubes_slab_*, csrc/marching_cubes.hip; nsr_ops.slab_windows / marching_cubes_streamed; slab_layers= of the
model's extractors): the entries and their refusals, which come before any launch and so run without a device; the window planner, whose windows must tile the
grid; and the Python-level refusals, which come before anything is computed.  The GPU tier (tests/test_gpu_mesh_streamed.py) compares the streamed mesh with the
dense one bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

NAMES = ("ac_marching_cubes_slab_scratch", "ac_marching_cubes_slab_count", "ac_marching_cubes_slab_emit")


def test_the_three_entries_are_declared_and_bound():
    from avatarcraft_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avatarcraft_hip.h")).read()
    for name, ret, arity in zip(NAMES, ("size_t", "int", "int"), (3, 11, 19)):
        assert name in _lib.EXPORTS and re.search(r"\b%s %s\s*\(" % (ret, name), hdr)
        assert len(_lib._SIGS[name][0]) == arity
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == arity              # the header's parameter list and the binding's agree
    assert _lib.lib().ac_version() == 10


def test_slab_scratch_is_a_host_function_and_the_dense_limit_stands():
    from avatarcraft_amd import _lib
    lib = _lib.lib()
    sc = lib.ac_marching_cubes_slab_scratch
    assert sc(2, 8, 8) == 0 and sc(3, 1, 8) == 0 and sc(3, 8, 1) == 0
    assert sc(2 ** 11, 2 ** 10, 2 ** 10) == 0 and sc(3, 2 ** 16, 2 ** 14) == 0                      # windows of 2^31 and more points
    assert sc(3, 2, 2) > 0
    big = sc(34, 2048, 2048)
    assert 5 * 34 * 2048 * 2048 <= big < 5.2 * 34 * 2048 * 2048                                     # 5 bytes per point of the WINDOW: 0.71 GB where the grid would take 43 GB
    assert sc(34, 2048, 2048) >= sc(33, 2048, 2048) >= sc(3, 2048, 2048)                            # a shorter window runs in a longer one's scratch
    assert lib.ac_marching_cubes_scratch(1296, 1296, 1296) == 0                                     # the limit of the dense route this works around
    assert lib.ac_marching_cubes_scratch(1290, 1290, 1290) > 0


def test_count_and_emit_refuse_before_any_launch():
    """AC_ERR_BAD_ARG (1) comes back before a buffer is touched or anything is launched: this runs without a device (the addresses are never read)"""
    from avatarcraft_amd import _lib
    lib = _lib.lib()
    P = 4096                                                     # a non-NULL address that nothing dereferences
    d3 = ctypes.c_double * 3
    one, zero = d3(1.0, 1.0, 1.0), d3(0.0, 0.0, 0.0)
    need = lib.ac_marching_cubes_slab_scratch(4, 8, 8)

    def count(window=P, n=4, ny=8, nz=8, first=0, last=0, scratch=P, nbytes=need, counts=P):
        return lib.ac_marching_cubes_slab_count(window, n, ny, nz, 0.0, first, last, scratch, nbytes, counts, None)

    def emit(window=P, n=4, ny=8, nz=8, first=0, last=0, scratch=P, nbytes=need, x0=6, den=1.0, span=one, lo=zero, v=P, nv=1, t=P, nt=1):
        return lib.ac_marching_cubes_slab_emit(window, n, ny, nz, 0.0, first, last, scratch, nbytes, x0, 0, den, span, lo, v, nv, t, nt, None)
    for fn in (count, emit):
        for kw, match in ((dict(n=2), "unsupported"), (dict(n=2, first=1), "unsupported"), (dict(n=2, last=1), "unsupported"), (dict(n=1, first=1, last=1), "unsupported"),
                          (dict(ny=1), "unsupported"), (dict(nz=1), "unsupported"), (dict(n=2 ** 11, ny=2 ** 10, nz=2 ** 10, nbytes=2 ** 40), "2\\^31"),
                          (dict(window=None), "NULL"), (dict(scratch=None), "NULL"), (dict(nbytes=need - 1), "scratch of %d bytes needed" % need)):
            assert fn(**kw) == 1, (fn.__name__, kw)
            assert re.search(match, lib.ac_last_error().decode()), (kw, lib.ac_last_error())
    assert count(counts=None) == 1 and b"NULL" in lib.ac_last_error()
    for kw in (dict(den=0.0), dict(span=None), dict(lo=None), dict(v=None), dict(t=None)):
        assert emit(**kw) == 1 and b"NULL buffer or den == 0" in lib.ac_last_error(), kw
    assert emit(x0=2 ** 32 - 3) == 1 and b"overflows 32 bits" in lib.ac_last_error()
    assert emit(first=1, x0=6) == 1 and b"x0 != 0" in lib.ac_last_error()


def _emitted(w):
    x0, n, first, last, _, _ = w
    verts = list(range(x0 + (0 if first else 1), x0 + (n if last else n - 1)))
    cells = list(range(x0, x0 + (n - 1 if last else n - 2)))
    return verts, cells


@pytest.mark.parametrize("slab_layers", [2, 3, 16, 17, 32])
def test_the_planners_windows_tile_the_grid(slab_layers):
    from avatarcraft_amd.nsr_ops import slab_windows
    for nx in range(2, 71):
        wins = slab_windows(nx, slab_layers)
        verts, cells, new = [], [], []
        for i, w in enumerate(wins):
            x0, n, first, last, new_lo, new_n = w
            v, c = _emitted(w)
            verts += v; cells += c
            new += list(range(x0 + new_lo, x0 + new_lo + new_n))
            assert 2 <= n <= slab_layers + 2 and x0 + n <= nx and new_lo + new_n == n
            assert first == (i == 0) and last == (i == len(wins) - 1) == (x0 + n == nx)
            if i == 0:
                assert x0 == 0 and new_lo == 0 and n == min(slab_layers, nx)
            else:
                assert x0 == wins[i - 1][0] + wins[i - 1][1] - 2 and new_lo == 2 and 1 <= new_n <= slab_layers
            if not last:
                assert new_n == slab_layers                                      # every request but the last is for slab_layers layers
        assert verts == list(range(nx)) and cells == list(range(nx - 1)) and new == list(range(nx)), (nx, slab_layers)
        assert sum(w[2] for w in wins) == 1 and sum(w[3] for w in wins) == 1
        if nx <= slab_layers:
            assert wins == [(0, nx, True, True, 0, nx)]
    for bad in (1, 0, 2.5, True, None):
        with pytest.raises(RuntimeError, match="slab_layers"):
            slab_windows(16, bad)
    with pytest.raises(RuntimeError, match="nx"):
        slab_windows(1, 4)


def test_python_refuses_before_anything_is_computed():
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    calls = []
    fill = lambda x0, out: calls.append(x0)
    for bad in (1, 0, 2.5):
        with pytest.raises(RuntimeError, match="slab_layers"):
            nsr_ops.marching_cubes_streamed(fill, 8, 8, 8, slab_layers=bad)
    with pytest.raises(RuntimeError, match="not a GPU"):
        nsr_ops.marching_cubes_streamed(fill, 8, 8, 8, slab_layers=4, device="cpu")                 # CPU tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="not a GPU"):
        nsr_ops.marching_cubes_streamed(fill, 8, 8, 8, slab_layers=4, device=torch.zeros(1).device)
    with pytest.raises(RuntimeError, match="callable"):
        nsr_ops.marching_cubes_streamed(torch.zeros(8, 8, 8), 8, 8, 8, slab_layers=4)
    with pytest.raises(RuntimeError, match="ny"):
        nsr_ops.marching_cubes_streamed(fill, 8, 1, 8, slab_layers=4)
    with pytest.raises(RuntimeError, match="den != 0"):
        nsr_ops.marching_cubes_streamed(fill, 8, 8, 8, slab_layers=4, den=0.0)
    with pytest.raises(RuntimeError, match=r"reaches 2\^31: lower slab_layers \(510\)"):
        nsr_ops.marching_cubes_streamed(fill, 2048, 2048, 2048, slab_layers=510)                     # 512 x 2048 x 2048 = 2^31
    assert calls == []
    torch.manual_seed(0)
    net = NeRFNetwork()                                                                              # on the CPU
    with pytest.raises(RuntimeError, match="never whole"):
        net.extract_fields_device(1.6, 16, slab_layers=16)
    for call in (lambda s: net.extract_geometry(1.6, 16, slab_layers=s), lambda s: net.extract_colored_mesh(1.6, 16, slab_layers=s),
                 lambda s: net.extract_textured_mesh(1.6, 16, texture_size=64, slab_layers=s)):
        for bad in (1, 0, 2.5):
            with pytest.raises(RuntimeError, match="slab_layers"):
                call(bad)
        with pytest.raises(RuntimeError, match="on the GPU"):
            call(16)
    with pytest.raises(RuntimeError, match="mesher='native'"):
        net.extract_geometry(1.6, 16, mesher="tetra", slab_layers=16)
