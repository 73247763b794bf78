"""CPU: the nsr_ops package keeps the public names nsr_ops.py had, the one scratch cache keeps the five sites' policies, and the occupancy
failure count survives a buffer that the cache lets go.  Needs neither the library nor a GPU."""
import ast
import importlib
import os
import pkgutil
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nsr_ops_public_names():
    """vars(nsr_ops) without underscore names and modules against tests/golden/nsr_ops_names.txt: the names nsr_ops.py bound before it became a package
    (written from that module, the library modules it happened to expose included)."""
    from avatarcraft_amd import nsr_ops
    was = set(open(os.path.join(ROOT, "tests", "golden", "nsr_ops_names.txt")).read().split())
    now = {k for k, v in vars(nsr_ops).items() if not k.startswith("_") and not isinstance(v, types.ModuleType)}
    library_modules = {"collections", "os", "np", "torch", "C", "L"}
    assert now - was == set()
    assert (was - now) - library_modules == {"ACCUMULATE_TABLE_GRAD_IN_PLACE", "SURFACE_WARPED_OUTPUTS"}
    for name in ("_chk", "_render_opts", "_SdfStencil"):                 # the private names used from outside the package
        assert getattr(nsr_ops, name) is not None
    # every public name is defined (def, class or assignment at module level) in exactly one submodule, and the package binds that object
    subs = [importlib.import_module(f"{nsr_ops.__name__}.{m.name}") for m in pkgutil.iter_modules(nsr_ops.__path__)]
    assert len(subs) == 8
    defined = {}
    for m in subs:
        for node in ast.parse(open(m.__file__).read()).body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                defined.setdefault(node.name, []).append(m)
            elif isinstance(node, ast.Assign):
                for tgt in node.targets:
                    for n in (tgt.elts if isinstance(tgt, ast.Tuple) else [tgt]):
                        defined.setdefault(n.id, []).append(m)
    for name in sorted(now) + ["_chk", "_render_opts", "_SdfStencil"]:
        assert len(defined.get(name, [])) == 1, (name, defined.get(name))
        assert vars(defined[name][0])[name] is getattr(nsr_ops, name), name
    assert not [n.id for n in ast.walk(ast.parse(open(nsr_ops.__file__).read())) if isinstance(n, ast.Name)]        # __init__ holds imports only


def test_stream_scratch_policies():
    from avatarcraft_amd._scratch import ScratchCache
    dropped = []
    c = ScratchCache(on_drop=dropped.append)
    assert c.get("a", 0, "cpu") is None and c.values() == []            # nothing asked for, nothing cached
    a = c.get("a", 64, "cpu")
    assert a.dtype == torch.uint8 and a.numel() == 64 and a.device.type == "cpu"
    assert c.get("a", 16, "cpu") is a and c.get("a", 64, "cpu") is a and c.get("a", 0, "cpu") is a      # a smaller request: the same buffer
    b = c.get("a", 65, "cpu")                                           # a larger one replaces it, and on_drop saw the old one
    assert b is not a and b.numel() == 65 and len(dropped) == 1 and dropped[0] is a and c.values() == [b]
    c.drop("nobody")                                                    # absent key: nothing happens
    assert len(dropped) == 1 and c.values() == [b]
    c.drop("a")
    assert dropped[1] is b and c.values() == [] and c.get("a", 0, "cpu") is None
    # zeroed
    z = ScratchCache(zeroed=True)
    assert not z.get(("cpu", 0), 4096, "cpu").any()
    z.clear()
    assert z.values() == []
    # the cap: a request that allocates while more than max_entries are held lets go of all of them, each seen once by on_drop
    dropped.clear()
    m = ScratchCache(zeroed=True, max_entries=2, on_drop=dropped.append)
    held = [m.get(k, 8, "cpu") for k in range(3)]
    assert dropped == [] and len(m.values()) == 3                       # (held > max_entries only shows at the next miss, as at the two capped sites)
    assert m.get(1, 8, "cpu") is held[1] and dropped == []              # a hit never evicts
    new = m.get(3, 8, "cpu")
    assert len(dropped) == 3 and all(any(d is h for d in dropped) for h in held) and m.values() == [new]
    m.clear()
    assert len(dropped) == 4 and dropped[3] is new


def test_occupancy_failure_count_survives_dropped_buffers(monkeypatch):
    """a buffer of the training-form cache whose sticky word (bytes 32..36) holds 3 is let go through the cache: the process total keeps the 3.
    The total is the process's: it is put back afterwards (other tests assert 0 failures), and both buffers are gone from the caches by the end."""
    from avatarcraft_amd import nsr_ops
    from avatarcraft_amd.nsr_ops import occupancy
    monkeypatch.setitem(occupancy._OCC_FAILURES, "dropped", occupancy._OCC_FAILURES["dropped"])
    key = ("cpu", 0, 7, 11)
    before = nsr_ops.occupancy_launch_failures()
    sc = occupancy._OT_SCRATCH.get(key, 64, "cpu")
    assert not sc.any()
    sc[32:36].view(torch.int32)[0] = 3
    assert nsr_ops.occupancy_launch_failures() == before + 3            # counted while it is held ...
    occupancy._OT_SCRATCH.drop(key)
    assert all(v is not sc for v in occupancy._OT_SCRATCH.values())
    assert nsr_ops.occupancy_launch_failures() == before + 3            # ... and after it is gone
    sc = occupancy._OP_SCRATCH.get(("cpu", 0), 64, "cpu")              # the inference form: replaced by a larger buffer
    sc[32:36].view(torch.int32)[0] = 2
    occupancy._OP_SCRATCH.get(("cpu", 0), 128, "cpu")
    assert nsr_ops.occupancy_launch_failures() == before + 5
    occupancy._OP_SCRATCH.drop(("cpu", 0))
    assert nsr_ops.occupancy_launch_failures() == before + 5


def test_typed_argument_check_on_cpu_tensors():
    """the helper of the typed checks: on a CPU tensor only its first refusal is reachable, with the caller's words"""
    from avatarcraft_amd.nsr_ops import _args
    with pytest.raises(RuntimeError, match="^vertices must be a CUDA tensor$"):
        _args._chk_typed(torch.zeros(4, 3, dtype=torch.float64), torch.float64, (None, 3), "typed", cuda_msg="vertices must be a CUDA tensor")
    with pytest.raises(RuntimeError, match="^both$"):
        _args._chk_cuda("both", torch.zeros(1), None)
    assert _args._chk_int(5, "m", 2) == 5 and _args._chk_int(2 ** 31 - 1, "m", 0, 2 ** 31) == 2 ** 31 - 1
    for bad in (True, 2.0, "3", 1, None):
        with pytest.raises(RuntimeError, match="^m$"):
            _args._chk_int(bad, "m", 2)
    with pytest.raises(RuntimeError, match="^m$"):
        _args._chk_int(2 ** 31, "m", 0, 2 ** 31)
