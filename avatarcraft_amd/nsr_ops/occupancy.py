"""The occupancy-grid renderers (NeRFRenderer.run_cuda in one launch: inference and training form) with the accounting of their barrier time-outs, and
the density-grid update that feeds them."""
import ctypes as C
import os

import torch

from .. import _lib as L
from .._scratch import ScratchCache
from ._args import _chk, _chk_typed, _f32, _inv_s_arg, _ray_args

# from this ray count on the inference launch runs in phases (same bits): 1.01 against 1.94 ms on a 256 x 256 view, 0.54 against 0.87 ms on a 4096-ray batch of
# its middle rows; a few dozen rays are quicker through the one-wave-per-group kernel (no grid barriers)
OCCUPANCY_PHASED_MIN_RAYS = 2048

# The phased kernels (inference and training form) synchronise their grid with barriers in global memory.  The launch is sized and checked for co-residency
# (csrc/ac_common.hpp: launch_resident); what is left is a FOREIGN kernel holding compute units for longer than a barrier's bounded spin -- then the launch
# gives up and counts itself in its scratch's sticky word.  Neither form hands out the partial result (the reference's loop, raymarching/raymarching.py:136-188,
# cannot produce one):
#   inference -- on the device: ac_render_rays_occupancy_phased queues the barrier-free kernel behind the phased one, conditional on that launch's verdict
#       word (a few microseconds when it is not needed, no host round trip); it renders every ray again, the same bits;
#   training form -- OCCUPANCY_VERIFY (default on; AC_OCC_VERIFY=0 for callers that poll occupancy_launch_failures() themselves): the wrapper reads the
#       sticky word behind the launch (one 4-byte read-back, +0.08 ms on a 0.34 ms launch) and raises OccupancyBarrierTimeout, which instant_nsr.run_cuda
#       answers with the chain of operators (the same pixels).
OCCUPANCY_VERIFY = os.environ.get("AC_OCC_VERIFY", "1") != "0"
_OCC_FAILURES = {"dropped": 0, "fallbacks": 0}        # sticky words of scratch buffers that were dropped or replaced | launches answered by the fallback


class OccupancyBarrierTimeout(RuntimeError):
    """a grid barrier of a phased occupancy launch timed out (compute units held by a foreign kernel): its outputs are partial and were NOT returned"""


def _sticky_word(sc):
    return int(sc[32:36].view(torch.int32).item())


def _keep_failures(sc):
    """a scratch buffer is let go: its failure count stays in the process total (clearing or re-allocating a buffer lost its sticky word)"""
    _OCC_FAILURES["dropped"] += _sticky_word(sc)


# zeroed once: every launch re-arms its sync words.  Inference form: one buffer per (device, stream), grown to the largest launch seen.  Training form: one
# per (device, stream, N, capacity) -- the layout depends on both, a buffer is re-armed for calls of ITS shape -- and all let go once more than 8 are held.
_OP_SCRATCH = ScratchCache(zeroed=True, on_drop=_keep_failures)
_OT_SCRATCH = ScratchCache(zeroed=True, max_entries=8, on_drop=_keep_failures)


def _occupancy_args(who, rays_o, rays_d, density_grid):
    """-> (rays_o [N,3], rays_d [N,3], density_grid [H,H,H]), checked: what the two occupancy renderers ask of their rays and grid"""
    rays_o, rays_d = _ray_args(rays_o, rays_d)
    grid = _chk(density_grid, "density_grid")
    if grid.dim() != 3 or grid.shape[0] != grid.shape[1] or grid.shape[0] != grid.shape[2]:
        raise RuntimeError(f"{who}: density_grid must be [H, H, H]")
    return rays_o, rays_d, grid


def render_rays_occupancy(field, rays_o, rays_d, density_grid, mean_density, bound, eps, inv_s, cos_anneal_ratio=1.0, count_samples=False, max_steps=0,
                          phased=None):
    """ac_render_rays_occupancy / ac_render_rays_occupancy_phased: the inference form of run_cuda in one launch (no host round trips).
    -> dict(weights_sum [N], depth [N] (raw sum of w t), image [N,3] (no background), normal_map [N,3] (+ n_samples, a [1] int32 device tensor))
    max_steps: a ray stops after that many samples (0 = no cap); see include/avatarcraft_hip.h for how that relates to the loop of rounds.
    phased: None = by ray count (OCCUPANCY_PHASED_MIN_RAYS); the two kernels give the same bits."""
    rays_o, rays_d, grid = _occupancy_args("render_rays_occupancy", rays_o, rays_d, density_grid)
    N, dev = rays_o.shape[0], rays_o.device
    out = dict(weights_sum=_f32(dev, N), depth=_f32(dev, N), image=_f32(dev, N, 3), normal_map=_f32(dev, N, 3))
    if count_samples:
        out["n_samples"] = torch.zeros(1, dtype=torch.int32, device=dev)
    inv_f, inv_t = _inv_s_arg(inv_s)
    args = (C.byref(field.c), rays_o.data_ptr(), rays_d.data_ptr(), N, grid.data_ptr(), int(grid.shape[0]), float(mean_density), float(bound), float(eps),
            inv_f, L.ptr(inv_t), float(cos_anneal_ratio), out["weights_sum"].data_ptr(), out["depth"].data_ptr(), out["image"].data_ptr(),
            out["normal_map"].data_ptr(), L.ptr(out.get("n_samples")), max(0, int(max_steps)))       # what the two entry points share
    if phased is None:
        phased = N >= OCCUPANCY_PHASED_MIN_RAYS
    if phased and N > 0:
        need = int(L.lib().ac_render_rays_occupancy_phased_scratch(N))
        sc = _OP_SCRATCH.get((str(dev), int(L.current_stream(dev) or 0)), need, dev)
        L.check(L.lib().ac_render_rays_occupancy_phased(*args, sc.data_ptr(), sc.numel(), L.current_stream(dev)), "render_rays_occupancy_phased")
        # (a launch whose grid barrier timed out is answered ON THE DEVICE: the library queues the barrier-free kernel behind the phased one, conditional on that
        #  launch's verdict word -- no read-back here, never a partial result; occupancy_launch_failures() counts such launches)
        return out
    L.check(L.lib().ac_render_rays_occupancy(*args, L.current_stream(dev)), "render_rays_occupancy")
    return out


def render_rays_occupancy_train(field, rays_o, rays_d, density_grid, mean_density, bound, eps, inv_s, cos_anneal_ratio=1.0, perturb=False, capacity=0,
                                composite_capacity=0, counter=None, bg=None):
    """ac_render_rays_occupancy_train: the training form of run_cuda without autograd in one launch (walk + record, offsets + packed samples, field on
    tiles dealt to all waves, the packed compositor per ray; grid barriers between the phases).  capacity / composite_capacity: the M of march_rays_train /
    composite_rays_train, both > 0 (a budgeted call: the packed layout lives in the launch's scratch); counter: the [2] int32 step counter (+= samples,
    += N); bg: None (raw sums), a number, a [3] / [1,3] or an [N,3] tensor -- image + (1 - weights_sum) * bg.
    -> dict(weights_sum [N], image [N,3], normal_map [N,3], gradient_error [1])"""
    rays_o, rays_d, grid = _occupancy_args("render_rays_occupancy_train", rays_o, rays_d, density_grid)
    N, dev = rays_o.shape[0], rays_o.device
    if counter is not None:
        msg = "render_rays_occupancy_train: counter must be a contiguous [2] int32 device tensor"
        if _chk_typed(counter, torch.int32, None, msg, cuda_msg=msg).numel() < 2:
            raise RuntimeError(msg)
    cap, ccap = int(capacity), int(composite_capacity) or int(capacity)
    if cap <= 0:
        raise RuntimeError("render_rays_occupancy_train: capacity must be > 0 (the un-budgeted form of march_rays_train sizes its layout after counting: use the operators)")
    bg_mode, bg_value, bg_t = 0, 0.0, None
    if bg is not None:
        if isinstance(bg, torch.Tensor):
            if bg.numel() == 1 and not bg.is_cuda:
                bg_mode, bg_value = 1, float(bg.reshape(()).item())
            elif bg.numel() == 1:                                  # a device scalar: as a broadcast triple, without a read-back
                bg_mode, bg_t = 2, _chk(bg.reshape(1).expand(3).contiguous(), "bg")
            elif bg.numel() == 3:
                bg_mode, bg_t = 2, _chk(bg.reshape(3), "bg")
            elif bg.numel() == 3 * N:
                bg_mode, bg_t = 3, _chk(bg.reshape(N, 3), "bg")
            else:
                raise RuntimeError(f"render_rays_occupancy_train: background of {tuple(bg.shape)} for {N} rays")
        else:
            bg_mode, bg_value = 1, float(bg)
    out = dict(weights_sum=_f32(dev, N), image=_f32(dev, N, 3), normal_map=_f32(dev, N, 3), gradient_error=_f32(dev, 1))
    need = int(L.lib().ac_render_rays_occupancy_train_scratch(N, cap))
    key = (str(dev), int(L.current_stream(dev) or 0), N, cap)      # (the layout depends on N and the capacity: a buffer is re-armed for calls of ITS shape)
    sc = _OT_SCRATCH.get(key, need, dev)
    inv_f, inv_t = _inv_s_arg(inv_s)
    L.check(L.lib().ac_render_rays_occupancy_train(C.byref(field.c), rays_o.data_ptr(), rays_d.data_ptr(), N, grid.data_ptr(), int(grid.shape[0]),
                                                   float(mean_density), float(bound), float(eps), inv_f, L.ptr(inv_t), float(cos_anneal_ratio),
                                                   1 if perturb else 0, cap, ccap, L.ptr(counter), L.ptr(bg_t), bg_mode, float(bg_value),
                                                   out["weights_sum"].data_ptr(), out["image"].data_ptr(), out["normal_map"].data_ptr(),
                                                   out["gradient_error"].data_ptr(), sc.data_ptr(), sc.numel(), L.current_stream(dev)),
            "render_rays_occupancy_train")
    if OCCUPANCY_VERIFY and N > 0 and _sticky_word(sc) != 0:
        _OT_SCRATCH.drop(key)               # (phases after the failed barrier were skipped: the buffer is not re-armed)
        _OCC_FAILURES["fallbacks"] += 1
        raise OccupancyBarrierTimeout("render_rays_occupancy_train: a grid barrier timed out (compute units held by a foreign kernel); no outputs were returned -- "
                                      "render through the operators (instant_nsr.run_cuda does)")
    return out


def occupancy_launch_failures():
    """launches of the phased occupancy kernels (inference and training form) whose grid barrier timed out, over the life of this process: the sticky word 8
    of every scratch buffer held now + the words of the buffers dropped or replaced since (kept in _OCC_FAILURES).  0 on a healthy run.  With
    OCCUPANCY_VERIFY (default) every one of them was answered by the barrier-free path and no partial result left the wrappers; without it such a launch leaves
    NaN in gradient_error / weights_sum[0].  Synchronises."""
    n = _OCC_FAILURES["dropped"]
    for sc in _OT_SCRATCH.values() + _OP_SCRATCH.values():
        n += _sticky_word(sc)
    return n


def occupancy_fallbacks():
    """phased launches whose outputs were withheld and rendered again / raised (OCCUPANCY_VERIFY)"""
    return _OCC_FAILURES["fallbacks"]


def debug_hold_cus(blocks, lds_bytes, millis, stream=None):
    """test utility: ac_debug_hold_cus on `stream` (a torch.cuda.Stream; default: the current one)"""
    st = stream.cuda_stream if stream is not None else L.current_stream(None)
    L.check(L.lib().ac_debug_hold_cus(int(blocks), int(lds_bytes), int(millis), st), "debug_hold_cus")


_DG_SCRATCH = ScratchCache(zeroed=True, max_entries=16)         # zeroed once: the launch re-arms its ticket; one buffer per (device, stream, H)


def density_grid_update(field, axis, grid, bound, inv_s=512.0, decay=0.95):
    """ac_density_grid_update: the grid update of update_extra_state (models/instant_nsr.py:303-346) in one launch, IN PLACE on grid [H,H,H];
    axis = torch.linspace(-bound, bound, H) on the device.  -> mean(grid) as a [1] float64 device tensor."""
    axis = _chk(axis.reshape(-1), "axis"); grid = _chk(grid, "density_grid")
    H = axis.shape[0]
    if tuple(grid.shape) != (H, H, H):
        raise RuntimeError("density_grid_update: grid must be [H, H, H] with H = len(axis)")
    dev = grid.device
    need = int(L.lib().ac_density_grid_update_scratch(H))
    if need == 0:
        raise RuntimeError(f"density_grid_update: H = {H} unsupported (2 <= H <= 1024)")
    sc = _DG_SCRATCH.get((str(dev), int(L.current_stream(dev) or 0), H), need, dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    L.check(L.lib().ac_density_grid_update(C.byref(field.c), axis.data_ptr(), H, float(bound), float(inv_s), float(decay), grid.data_ptr(), mean.data_ptr(),
                                           sc.data_ptr(), need, L.current_stream(dev)), "density_grid_update")
    return mean
