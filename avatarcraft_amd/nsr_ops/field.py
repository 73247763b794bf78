"""The field as the kernels see it: the parameter snapshot (Field), the packed layout of its parameter gradients, the view-direction columns of the
colour layer, and the launches that evaluate or differentiate the field alone (no rays): SDF, colour, packed samples, variance, weight norm."""
import collections
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._args import _F32, _chk, _f32, _inv_s_arg


class Field:
    """Device-resident parameters of the default NeRFNetwork in the layout ac_field wants:
    table [n_entries,2], offsets (17 host ints), S=log2(per_level_scale), H, and the EFFECTIVE
    (weight-normed) MLP matrices W1[64,35] b1[64] W2[16,64] b2[16] Wc1[64,21] Wc2[64,64] Wc3[3,64]."""

    def __init__(self, table, offsets, per_level_scale, base_resolution, W1, b1, W2, b2, Wc1, Wc2, Wc3, Wc1_sh=None):
        """Wc1_sh [64,16] (optional): NeRFNetwork(use_viewdirs=True) -- the columns of the effective color_net.0 weight that multiply the 16 spherical
        harmonics of the ray direction (columns 3..18 of its [64,37] matrix; Wc1 then holds the other 21: x, normal, geo_feat).  See ac_field.Wc1_sh."""
        offsets = [int(v) for v in offsets]
        if len(offsets) != 17:
            raise RuntimeError("the fused renderer supports the 16-level hash grid only")
        self.t = dict(table=_chk(table, "table", (offsets[-1], 2)), W1=_chk(W1, "W1", (64, 35)), b1=_chk(b1, "b1", (64,)),
                      W2=_chk(W2, "W2", (16, 64)), b2=_chk(b2, "b2", (16,)), Wc1=_chk(Wc1, "Wc1", (64, 21)),
                      Wc2=_chk(Wc2, "Wc2", (64, 64)), Wc3=_chk(Wc3, "Wc3", (3, 64)))
        self.S = float(np.float32(np.log2(per_level_scale)))
        self.H = int(base_resolution)
        f = L.ac_field()
        f.table = self.t["table"].data_ptr()
        for i, v in enumerate(offsets):
            f.offsets[i] = v
        f.S = self.S
        f.H = self.H
        for k in ("W1", "b1", "W2", "b2", "Wc1", "Wc2", "Wc3"):
            setattr(f, k, self.t[k].data_ptr())
        if Wc1_sh is not None:
            self.t["Wc1_sh"] = _chk(Wc1_sh, "Wc1_sh", (64, 16))
            f.Wc1_sh = self.t["Wc1_sh"].data_ptr()
        self.has_viewdirs = Wc1_sh is not None
        self.c = f
        self.device = table.device
        self.prepared = None
        self._half = None

    @classmethod
    def sdf_only(cls, table, offsets, per_level_scale, base_resolution, W1, b1, W2, b2):
        """the SDF side only (zero colour matrices): what the sampling stage and the SDF-query operator read"""
        dev = table.device
        return cls(table, offsets, per_level_scale, base_resolution, W1, b1, W2, b2, _f32(dev, 64, 21, zero=True), _f32(dev, 64, 64, zero=True),
                   _f32(dev, 3, 64, zero=True))

    @classmethod
    def color_only(cls, Wc1, Wc2, Wc3):
        """the colour side only: zero SDF matrices and a dummy 16-level layout of one entry per level (the colour kernels never touch the table)"""
        dev = Wc1.device
        return cls(_f32(dev, 16, 2, zero=True), list(range(0, 17)), 2.0, 16, _f32(dev, 64, 35, zero=True), _f32(dev, 64, zero=True),
                   _f32(dev, 16, 64, zero=True), _f32(dev, 16, zero=True), Wc1, Wc2, Wc3)

    def half_table(self):
        """the hash table in half precision (ac_table_to_half): an int32 [n_entries] device tensor, one dword per entry (channel 0 in the low half), 4
        bytes per entry instead of 8.  Made once per Field -- a Field is a snapshot of the parameters, a changed table gets a new Field -- and what
        render_rays(table_dtype="half") gathers from.  RuntimeError if a finite value of the table does not fit fp16 (it would render as inf)."""
        if self._half is None:
            table = self.t["table"]
            n = table.shape[0]
            h = torch.empty((n,), dtype=torch.int32, device=self.device)
            n_bad = torch.zeros((1,), dtype=torch.int32, device=self.device)
            L.check(L.lib().ac_table_to_half(table.data_ptr(), n, h.data_ptr(), n_bad.data_ptr(), L.current_stream(self.device)), "table_to_half")
            bad = int(n_bad.item())
            if bad:
                raise RuntimeError(f"half_table: {bad} of {n} table entries hold a finite value beyond the fp16 range (|v| > 65504 becomes inf): "
                                   f"this field cannot be rendered from a half-precision table")
            self._half = h
        return self._half

    def prepare(self):
        """ac_field_prepare: lay the weights out once in the order the renderer keeps them in LDS (its 512 workgroups per launch then copy
        the image linearly).  Call again whenever a parameter tensor of this Field is modified in place."""
        if self.prepared is None:
            self.prepared = torch.empty(L.FIELD_PREPARED_BYTES, dtype=torch.uint8, device=self.device)
        self.c.prepared = None
        L.check(L.lib().ac_field_prepare(C.byref(self.c), self.prepared.data_ptr(), L.current_stream(self.device)), "field_prepare")
        self.c.prepared = self.prepared.data_ptr()
        return self


# The packed parameter gradients of the training kernels (include/avatarcraft_hip.h), w.r.t. the EFFECTIVE matrices:
#   g_sdf_params   = dW1 [64][36] (column 35 = db1) | dW2 [16][64] | db2 [16]                        (render core backward, SDF-stencil backward)
#   g_color_params = dWc1 [64][32] (columns 0..20) | dWc2 [64][64] | dWc3 [16][64] (rows 0..2)       (render core backward, colour backward)
# THE definition on this side: per tensor its element offset in the vector, the stride between its rows and its shape.
PackedSlot = collections.namedtuple("PackedSlot", "offset stride shape")
SDF_PARAM_GRADS = dict(W1=PackedSlot(0, 36, (64, 35)), b1=PackedSlot(35, 36, (64,)), W2=PackedSlot(64 * 36, 64, (16, 64)),
                       b2=PackedSlot(64 * 36 + 16 * 64, 1, (16,)))
SDF_PARAM_GRADS_LEN = 64 * 36 + 16 * 64 + 16
COLOR_PARAM_GRADS = dict(Wc1=PackedSlot(0, 32, (64, 21)), Wc2=PackedSlot(64 * 32, 64, (64, 64)), Wc3=PackedSlot(64 * 32 + 64 * 64, 64, (3, 64)))
COLOR_PARAM_GRADS_LEN = 64 * 32 + 64 * 64 + 16 * 64


def _split_packed(g, slots, length):
    if g.dim() != 1 or g.shape[0] != length or not g.is_contiguous():
        raise RuntimeError(f"a packed parameter gradient of {length} contiguous elements, got {tuple(g.shape)}")
    return tuple(g.as_strided(s.shape, (s.stride, 1)[:len(s.shape)], g.storage_offset() + s.offset) for s in slots.values())


def split_sdf_param_grads(g):
    """g_sdf_params [SDF_PARAM_GRADS_LEN] -> (dW1 [64,35], db1 [64], dW2 [16,64], db2 [16]), views of g"""
    return _split_packed(g, SDF_PARAM_GRADS, SDF_PARAM_GRADS_LEN)


def split_color_param_grads(g):
    """g_color_params [COLOR_PARAM_GRADS_LEN] -> (dWc1 [64,21], dWc2 [64,64], dWc3 [3,64]), views of g"""
    return _split_packed(g, COLOR_PARAM_GRADS, COLOR_PARAM_GRADS_LEN)


VIEWDIR_COLS = 16                      # degree-4 spherical harmonics of the ray direction: columns 3 .. 18 of a use_viewdirs color_net.0 weight [64, 37]


def split_viewdir_weight(Wc1):
    """the effective color_net.0 weight of NeRFNetwork(use_viewdirs=True), [64, 37] = [x(3) | sh(d)(16) | normal(3) | geo_feat(15)] (models/instant_nsr.py:648-650)
    -> (Wc1 [64,21] = [x | normal | geo_feat] as the fused kernels keep it, Wc1_sh [64,16]); a [64,21] weight -> (Wc1, None)"""
    if Wc1.shape[1] == 21:
        return Wc1, None
    if Wc1.shape[1] != 21 + VIEWDIR_COLS:
        raise RuntimeError(f"colour layer 1 has {Wc1.shape[1]} inputs: the fused renderer takes 21 (no view directions) or 37 (degree-4 spherical harmonics)")
    return torch.cat([Wc1[:, :3], Wc1[:, 3 + VIEWDIR_COLS:]], dim=1).contiguous(), Wc1[:, 3:3 + VIEWDIR_COLS].contiguous()


def join_viewdir_grad(g21, g_sh):
    """inverse of split_viewdir_weight for gradients: ([64,21], [64,16]) -> [64,37]"""
    return torch.cat([g21[:, :3], g_sh, g21[:, 3:]], dim=1)


def sh_bias(field, rays_d, want_sh=True):
    """ac_sh_bias: the per-ray layer-1 bias of the colour network for the view directions rays_d [N,3] -> (bias [N,64], sh [N,16] or None)"""
    rays_d = _chk(rays_d.reshape(-1, 3), "rays_d")
    N, dev = rays_d.shape[0], rays_d.device
    bias, sh = _f32(dev, N, 64), _f32(dev, N, VIEWDIR_COLS) if want_sh else None
    L.check(L.lib().ac_sh_bias(C.byref(field.c), rays_d.data_ptr(), N, bias.data_ptr(), L.ptr(sh), L.current_stream(dev)), "sh_bias")
    return bias, sh


def weight_norm_forward(pairs, outs):
    """outs[i][r, :] = v[r, :] * g[r] / ||v[r, :]|| for every (v, g) in pairs, ONE launch (ac_weight_norm_forward); outs may be row-strided views"""
    n = len(pairs)
    arr = (L.ac_wn_layer * n)()
    for i, ((v, g), w) in enumerate(zip(pairs, outs)):
        assert v.is_contiguous() and g.is_contiguous() and v.dtype == _F32 and w.dtype == _F32 and w.stride(1) == 1 and tuple(w.shape) == tuple(v.shape)
        arr[i] = L.ac_wn_layer(v.data_ptr(), g.data_ptr(), w.data_ptr(), v.shape[0], v.shape[1], w.stride(0), 0)
    L.check(L.lib().ac_weight_norm_forward(arr, n, L.current_stream(pairs[0][0].device)), "weight_norm_forward")
    return outs


PG_WEIGHT_NORM, PG_ADD, PG_VARIANCE = 0, 1, 2


def param_grads(entries, device):
    """entries: (kind, src tensor / (tensor, element offset), src_stride, rows, cols, v, g, dst, dst2); everything ACCUMULATED into dst / dst2, ONE launch"""
    n = len(entries)
    arr = (L.ac_pg_entry * n)()
    keep = []
    for i, (kind, src, stride, rows, cols, v, g, dst, dst2) in enumerate(entries):
        off = 0
        if isinstance(src, tuple):
            src, off = src
        for t in (src, v, g, dst, dst2):
            assert t is None or (t.dtype == _F32 and t.is_contiguous())
        keep.append((src, v, g, dst, dst2))
        arr[i] = L.ac_pg_entry(src.data_ptr() + 4 * off, L.ptr(v), L.ptr(g), dst.data_ptr(), L.ptr(dst2), rows, cols, stride, kind)
    L.check(L.lib().ac_param_grads(arr, n, L.current_stream(device)), "param_grads")


def variance_forward(variance):
    """forward_variance() without a graph: clip(exp(10 * variance), 1e-6, 1e6) as a [1, 1] tensor, one launch (ac_variance_forward)"""
    v = variance.detach()
    _chk(v, "variance")
    if v.dtype != torch.float32 or v.numel() != 1:
        raise RuntimeError("variance_forward: a single float32 value")
    out = torch.empty((1, 1), dtype=torch.float32, device=v.device)
    L.check(L.lib().ac_variance_forward(v.data_ptr(), out.data_ptr(), L.current_stream(v.device)), "variance_forward")
    return out


def field_samples(field, xyzs, dirs, deltas, bound, eps, inv_s, cos_anneal_ratio=1.0, want_sdf=False, want_gradient=False):
    """ac_field_samples: the field on packed samples (what run_cuda evaluates between the marcher and the packed compositor).
    xyzs, dirs [M,3]; deltas [M] (march_rays_train) or [M,2] (march_rays; column 0 is the step).  inv_s: float or a CUDA tensor (read on the device).
    -> dict(alpha [M], rgb [M,3], normal [M,3] (+ sdf [M], gradient [M,3]))"""
    xyzs = _chk(xyzs.reshape(-1, 3), "xyzs"); dirs = _chk(dirs.reshape(-1, 3), "dirs"); deltas = _chk(deltas, "deltas")
    M, dev = xyzs.shape[0], xyzs.device
    if dirs.shape[0] != M or deltas.shape[0] != M or deltas.dim() not in (1, 2):
        raise RuntimeError("field_samples: xyzs [M,3], dirs [M,3], deltas [M] or [M,k]")
    stride = 1 if deltas.dim() == 1 else int(deltas.shape[1])
    out = dict(alpha=_f32(dev, M), rgb=_f32(dev, M, 3), normal=_f32(dev, M, 3))
    if want_sdf:
        out["sdf"] = _f32(dev, M)
    if want_gradient:
        out["gradient"] = _f32(dev, M, 3)
    inv_f, inv_t = _inv_s_arg(inv_s)
    L.check(L.lib().ac_field_samples(C.byref(field.c), xyzs.data_ptr(), dirs.data_ptr(), deltas.data_ptr(), stride, M, float(bound), float(eps), inv_f, L.ptr(inv_t),
                                     float(cos_anneal_ratio), out["alpha"].data_ptr(), out["rgb"].data_ptr(), out["normal"].data_ptr(),
                                     L.ptr(out.get("sdf")), L.ptr(out.get("gradient")), L.current_stream(dev)), "field_samples")
    return out


def field_sdf(field, x, bound):
    """forward_sdf (instant_nsr.py:627-642): x [B,3] -> [B,16] (sdf, 15 features)"""
    x = _chk(x.reshape(-1, 3), "x")
    out = _f32(x.device, x.shape[0], 16)
    L.check(L.lib().ac_field_sdf(C.byref(field.c), x.data_ptr(), x.shape[0], float(bound), out.data_ptr(),
                                 L.current_stream(x.device)), "field_sdf")
    return out


def field_color(field, x, n, sdfout, dirs=None):
    """forward_color (instant_nsr.py:644-663): -> rgb [B,3]; dirs [B,3] = the view direction of every point for a field with view directions"""
    x = _chk(x.reshape(-1, 3), "x"); n = _chk(n.reshape(-1, 3), "n"); sdfout = _chk(sdfout.reshape(-1, 16), "sdfout")
    if dirs is not None:
        dirs = _chk(dirs.reshape(-1, 3), "dirs", (x.shape[0], 3))
    out = _f32(x.device, x.shape[0], 3)
    L.check(L.lib().ac_field_color_dirs(C.byref(field.c), x.data_ptr(), L.ptr(dirs), n.data_ptr(), sdfout.data_ptr(), x.shape[0], out.data_ptr(),
                                        L.current_stream(x.device)), "field_color")
    return out
