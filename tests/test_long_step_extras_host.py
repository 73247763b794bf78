"""CPU tier of the long renderer's training options (GPU tier: tests/test_gpu_long_step_extras.py): the pair entry ac_render_rays_long_pair is declared,
exported and bound; save_stencil / opacity_only / table_dtype are checked before any device work; the model's switch exists and is off by default."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_pair_entry_is_declared_exported_and_bound():
    from avatarcraft_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "avatarcraft_hip.h")).read()
    assert re.search(r"\bint ac_render_rays_long_pair\s*\(", hdr)
    assert "ac_render_rays_long_pair" in _lib.EXPORTS
    # the same C signature as ac_render_rays_pair and ac_render_rays_long: (field, opts, rays_o, rays_d, bg2, noise2, lin_z, lin_u, out, stream)
    sig = lambda name: re.sub(r"\s+", " ", re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1))
    norm = lambda s: s.replace("bg2", "bg").replace("noise2", "noise")
    assert norm(sig("ac_render_rays_long_pair")) == norm(sig("ac_render_rays_pair")) == sig("ac_render_rays_long")
    assert _lib._SIGS["ac_render_rays_long_pair"] == _lib._SIGS["ac_render_rays_pair"] == _lib._SIGS["ac_render_rays_long"]
    lib = _lib.lib()                                   # (dlopen + symbol check: no GPU needed)
    assert hasattr(lib, "ac_render_rays_long_pair")
    # the header no longer states the old rule of the canonical entry, the posed entry keeps its own
    assert "feat7 must be NULL and opts->opacity_only / skip_masked must be 0" not in hdr
    assert "feat7 must be NULL and opts->opacity_only 0" in hdr


def test_raw_entry_names_its_rules_without_a_device():
    """the argument checks of the C entries run before any device call (an empty batch: the rules are checked first, the buffers are not touched)"""
    import ctypes as C
    from avatarcraft_amd import _lib as L
    lib = L.lib()
    f = L.ac_field()
    o = L.ac_render_out()
    keep = (C.c_float * 4)()
    o.feat7 = C.addressof(keep)
    mk = lambda T0, up, **kw: L.ac_render_opts(0, T0, up, 1.6, 1.0, 1.0, 0.005, 0, None, None, None, 0, 0, kw.get("opacity", 0))
    for entry in (lib.ac_render_rays_long, lib.ac_render_rays_long_pair):
        assert entry(C.byref(f), C.byref(mk(100, 64)), None, None, None, None, None, None, C.byref(o), None) != 0
        msg = lib.ac_last_error()
        assert b"feat7" in msg and b"multiple of 16" in msg and b"164" in msg, msg
        assert entry(C.byref(f), C.byref(mk(100, 64, opacity=2)), None, None, None, None, None, None, C.byref(L.ac_render_out()), None) != 0
        assert b"opacity_only must be 0 or 1" in lib.ac_last_error()
        assert entry(C.byref(f), C.byref(mk(400, 128)), None, None, None, None, None, None, C.byref(L.ac_render_out()), None) != 0
        assert b"<= 512" in lib.ac_last_error()


def test_python_rules_need_no_device():
    from avatarcraft_amd import nsr_ops
    z = torch.zeros(4, 3)
    p = inspect.signature(nsr_ops.render_rays_long).parameters
    assert p["save_stencil"].default is False and p["opacity_only"].default is False
    assert inspect.signature(nsr_ops.render_rays_long_pair).parameters["save_stencil"].default is False
    # the pair wrapper mirrors render_rays_pair: the same parameters in the same order, then save_stencil
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(nsr_ops.render_rays_long_pair) == names(nsr_ops.render_rays_pair) + ["save_stencil"]
    with pytest.raises(RuntimeError, match=r"save_stencil \(feat7\) needs num_steps \+ upsample_steps a multiple of 16, got 100 \+ 64"):
        nsr_ops.render_rays_long(None, z, z, 100, 64, train_extras=True, save_stencil=True)
    with pytest.raises(RuntimeError, match=r"multiple of 16, got 100 \+ 64"):
        nsr_ops.render_rays_long_pair(None, z, z, torch.zeros(8, 100), 100, 64, save_stencil=True)
    with pytest.raises(RuntimeError, match="train_extras=True, no warp"):
        nsr_ops.render_rays_long(None, z, z, 128, 128, save_stencil=True)
    with pytest.raises(RuntimeError, match="train_extras=True, no warp"):
        nsr_ops.render_rays_long(None, z, z, 128, 128, train_extras=True, save_stencil=True, warp=object())
    with pytest.raises(RuntimeError, match="opacity_only"):
        nsr_ops.render_rays_long(None, z, z, 100, 64, warp=object(), opacity_only=True)
    for call in (lambda: nsr_ops.render_rays_long(None, z, z, 128, 128, table_dtype="half"),
                 lambda: nsr_ops.render_rays_long(None, z, z, 128, 128, opacity_only=True, table_dtype="half"),
                 lambda: nsr_ops.render_rays_long(None, z, z, 128, 128, train_extras=True, save_stencil=True, table_dtype="half"),
                 lambda: nsr_ops.render_rays_long_pair(None, z, z, torch.zeros(8, 128), 128, 128, table_dtype="half")):
        with pytest.raises(RuntimeError, match="table_dtype='half'"):
            call()
    with pytest.raises(RuntimeError, match="<= 512"):
        nsr_ops.render_rays_long_pair(None, z, z, torch.zeros(8, 400), 400, 128)
    with pytest.raises(RuntimeError, match="multiple"):
        nsr_ops.render_rays_long_pair(None, z, z, torch.zeros(8, 100), 100, 60)


def test_model_switch_is_opt_in():
    from avatarcraft_amd.instant_nsr import NeRFNetwork
    assert NeRFNetwork.long_step_extras is False
    net = NeRFNetwork.__new__(NeRFNetwork)             # (no parameters needed: the rule is a function of the switch and the counts)
    assert not net._long_save_stencil(128, 128)
    net.long_step_extras = True
    assert net._long_save_stencil(128, 128) and net._long_save_stencil(96, 32) and not net._long_save_stencil(100, 64)
