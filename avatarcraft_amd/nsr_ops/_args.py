"""What every wrapper of the package does to its arguments before a launch: the tensor checks (RuntimeError naming the argument, before any device work),
the float32 allocator, and the two argument forms several launches share (the ray pair, inv_s as a number or a device tensor)."""
import numpy as np
import torch

_F32 = torch.float32


def _chk(t, name, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != _F32:
        raise RuntimeError(f"{name} must be a float32 tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _chk_cuda(msg, *tensors):
    """RuntimeError(msg) unless every one of `tensors` is a CUDA tensor"""
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(msg)


def _chk_typed(t, dtypes, shape, msg, cuda_msg=None, device=None, contiguous=True):
    """the check of a tensor argument that is not plain float32 (that is _chk's), with the caller's wording: RuntimeError(cuda_msg) unless t is a CUDA tensor
    (None: not asked here), then RuntimeError(msg) unless t has the dtype (one of the dtypes) given, matches `shape` -- a tuple in which None is a free
    dimension; None: any shape --, is contiguous (contiguous="rows": unit stride along the last dimension is enough; False: not asked) and lives on
    `device` (None: not asked).  -> t"""
    if cuda_msg is not None:
        _chk_cuda(cuda_msg, t)
    ok = t.dtype in (dtypes if isinstance(dtypes, tuple) else (dtypes,))
    ok = ok and (shape is None or (t.dim() == len(shape) and all(s is None or s == n for s, n in zip(shape, t.shape))))
    ok = ok and (not contiguous or (t.stride(-1) == 1 if contiguous == "rows" else t.is_contiguous()))
    if not ok or (device is not None and t.device != device):
        raise RuntimeError(msg)
    return t


def _chk_int(v, msg, lo, hi=None):
    """RuntimeError(msg) unless v is an integer (a Python or numpy one, not a bool) with lo <= v (< hi).  -> int(v)"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v >= hi):
        raise RuntimeError(msg)
    return int(v)


def _f32(dev, *shape, zero=False):
    """an uninitialised (zero: a zeroed) float32 tensor of that shape on `dev`"""
    return (torch.zeros if zero else torch.empty)(shape, dtype=_F32, device=dev)


def _dc(t):
    return t.detach().contiguous()


def _inv_s_arg(inv_s):
    """(float for ac_render_opts.inv_s, device tensor or None for .inv_s_dev): a CUDA tensor (forward_variance()) is handed over as a
    pointer -- the trainable variance never takes a host round trip"""
    if isinstance(inv_s, torch.Tensor):
        if inv_s.is_cuda:
            t = inv_s.detach().reshape(-1)[:1].to(_F32).contiguous()
            return 0.0, t
        return float(inv_s.detach().reshape(-1)[0]), None
    return float(inv_s), None


def _ray_args(rays_o, rays_d):
    return _chk(rays_o.reshape(-1, 3), "rays_o"), _chk(rays_d.reshape(-1, 3), "rays_d")
