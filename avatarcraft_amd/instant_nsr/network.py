"""NeRFNetwork: the reference's constructor and torch forward functions (models/instant_nsr.py:478-718) on the renderer and its three mixins."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import nsr_ops
from ..encoder import get_encoder
from .renderer import NeRFRenderer, SingleVarianceNetwork
from .occupancy import OccupancyRendering
from .export import MeshExport
from .surface import SurfaceRendering


class NeRFNetwork(OccupancyRendering, MeshExport, SurfaceRendering, NeRFRenderer):
    """models/instant_nsr.py:478-718; the construction order (and therefore the RNG stream) follows the reference,
    so torch.manual_seed(s); NeRFNetwork() yields the same initial parameters."""

    def __init__(self, encoding="hashgrid", encoding_dir="sphere_harmonics", num_layers=2, hidden_dim=64, geo_feat_dim=15,
                 num_layers_color=3, hidden_dim_color=64, bound=1.0, geometric_init=True, weight_norm=True, cuda_ray=False,
                 include_input=True, curvature_loss=False, use_viewdirs=False):
        super().__init__(cuda_ray, curvature_loss)
        self.num_layers, self.hidden_dim, self.geo_feat_dim, self.include_input = num_layers, hidden_dim, geo_feat_dim, include_input
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.use_viewdirs = use_viewdirs
        pos_cfg = {"in_dim": 3, "freq_multires": 6, "hash_num_levels": 16, "hash_level_dim": 2, "hash_base_resolution": 16,
                   "hash_per_level_scale": 1.3819, "hash_log2_hashmap_size": 19, "hash_desired_resolution": 2048}
        dir_cfg = {"in_dim": 3, "freq_multires": 4}
        self.encoder, self.in_dim = get_encoder(encoding, pos_cfg)
        sdf_net = []
        for l in range(num_layers):
            in_dim = (self.in_dim + 3 if include_input else self.in_dim) if l == 0 else hidden_dim
            out_dim = 1 + geo_feat_dim if l == num_layers - 1 else hidden_dim
            lin = nn.Linear(in_dim, out_dim)
            if geometric_init:
                if l == num_layers - 1:
                    torch.nn.init.normal_(lin.weight, mean=np.sqrt(np.pi) / np.sqrt(in_dim), std=0.0001)
                    torch.nn.init.constant_(lin.bias, 0)
                elif l == 0 and include_input:
                    torch.nn.init.constant_(lin.bias, 0.0)
                    torch.nn.init.normal_(lin.weight[:, :3], 0.0, np.sqrt(2) / np.sqrt(out_dim))
                    torch.nn.init.constant_(lin.weight[:, 3:], 0.0)
                else:
                    torch.nn.init.constant_(lin.bias, 0.0)
                    torch.nn.init.normal_(lin.weight[:, :], 0.0, np.sqrt(2) / np.sqrt(out_dim))
            if weight_norm:
                lin = nn.utils.weight_norm(lin)
            sdf_net.append(lin)
        self.sdf_net = nn.ModuleList(sdf_net)
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color
        self.encoder_dir = None
        if use_viewdirs:
            self.encoder_dir, self.in_dim_color = get_encoder(encoding_dir, dir_cfg)
            self.in_dim_color = self.in_dim_color + geo_feat_dim + 6
        else:
            self.in_dim_color = geo_feat_dim + 6
        color_net = []
        for l in range(num_layers_color):
            lin = nn.Linear(self.in_dim_color if l == 0 else hidden_dim, 3 if l == num_layers_color - 1 else hidden_dim, bias=False)
            if weight_norm:
                lin = nn.utils.weight_norm(lin)
            color_net.append(lin)
        self.color_net = nn.ModuleList(color_net)
        self.deviation_net = SingleVarianceNetwork(0.3)
        self.activation = nn.Softplus(beta=100)

    # ---- differentiable field (autograd path: HIP hash encoder + torch MLP), reference :627-704
    def forward_sdf(self, x, bound):
        h = self.encoder(x, bound)
        if self.include_input:
            h = torch.cat([x, h], dim=-1)
        for l in range(self.num_layers):
            h = self.sdf_net[l](h)
            if l != self.num_layers - 1:
                h = self.activation(h)
        return h

    def forward_sdf_stencil(self, x, bound, epsilon):
        """forward_sdf(x) (:627-642) and finite_difference_normals_approximator(x) (:687-704) together: the seven hash encodings
        come from one stencil launch (encoder.forward_stencil) and the SDF MLP runs once over the 7B points.
        Returns (sdf_out [B,16], gradient [B,3])."""
        if self.fused_training and self._sdf_supported() and x.is_cuda:            # one kernel forward, two backward (csrc/sdf_stencil_train.hip)
            l0, l1, enc = self.sdf_net[0], self.sdf_net[1], self.encoder
            W = nsr_ops.weight_norm_all([l0, l1])                                   # the same effective matrices as every other fused path, bit for bit
            return nsr_ops.sdf_stencil(x, enc.embeddings, W[0], l0.bias, W[1], l1.bias, self._offsets_host(), enc.per_level_scale,
                                       enc.base_resolution, bound, epsilon)
        B = x.shape[0]
        h7 = self.encoder.forward_stencil(x, bound, epsilon)                       # [7,B,32]: x, +x, -x, +y, -y, +z, -z
        pts = x.unsqueeze(0).repeat(7, 1, 1)
        for k in range(3):
            pts[1 + 2 * k, :, k] = (x[:, k] + epsilon).clamp(-bound, bound)
            pts[2 + 2 * k, :, k] = (x[:, k] - epsilon).clamp(-bound, bound)
        h = torch.cat([pts, h7], dim=-1).reshape(7 * B, -1) if self.include_input else h7.reshape(7 * B, -1)
        for l in range(self.num_layers):
            h = self.sdf_net[l](h)
            if l != self.num_layers - 1:
                h = self.activation(h)
        h = h.view(7, B, -1)
        gradient = (0.5 * (h[1::2, :, 0] - h[2::2, :, 0]) / epsilon).t()
        return h[0], gradient

    def forward_color_fused(self, x, n, sdf_out):
        """forward_color on the outputs of forward_sdf (sdf_out [B,16] = [sdf, feat]) as one fused op with a fused backward"""
        W = nsr_ops.weight_norm_all(list(self.color_net))
        return nsr_ops.color_mlp(x, n, sdf_out, W[0], W[1], W[2])

    def forward_color(self, x, d, n, geo_feat, bound):
        if self.use_viewdirs:
            h = torch.cat([x, self.encoder_dir(d), n, geo_feat], dim=-1)
        else:
            h = torch.cat([x, n, geo_feat], dim=-1)
        for l in range(self.num_layers_color):
            h = self.color_net[l](h)
            if l != self.num_layers_color - 1:
                h = F.relu(h, inplace=True)
        return torch.sigmoid(h)

    def forward_variance(self):
        v = self.deviation_net.variance
        if not (torch.is_grad_enabled() and v.requires_grad):
            # no graph wanted: the value only changes with the parameter (five small launches per render otherwise; the frozen net_gt of the
            # stylisation step never changes at all)
            key = (v.data_ptr(), v._version, v.device)
            c = getattr(self, "_inv_s_cache", None)
            if c is None or c[0] != key:
                with torch.no_grad():
                    if v.is_cuda and v.dtype == torch.float32:
                        c = (key, nsr_ops.variance_forward(v))                       # one launch, the same bits (ac_variance_forward)
                    else:
                        c = (key, self.deviation_net(torch.zeros([1, 3]))[:, :1].clip(1e-6, 1e6))
                self._inv_s_cache = c
            return c[1]
        return self.deviation_net(torch.zeros([1, 3]))[:, :1].clip(1e-6, 1e6)

    def density(self, x, bound):
        """sdf only (reference :669-681); no-grad queries go through the fused field kernel"""
        if not torch.is_grad_enabled() and x.is_cuda and self._sdf_supported():
            return nsr_ops.field_sdf(self._field_for(), x.reshape(-1, 3).float().contiguous(), bound)[:, 0].reshape(x.shape[:-1])
        return self.forward_sdf(x, bound)[..., 0]

    def gradient(self, x, bound, epsilon=0.0005):
        return self.finite_difference_normals_approximator(x, bound, epsilon)

    def finite_difference_normals_approximator(self, x, bound, epsilon=0.0005):
        outs = []
        for k in range(3):
            e = torch.zeros(1, 3, device=x.device); e[0, k] = epsilon
            pos = self.forward_sdf((x + e).clamp(-bound, bound), bound)[:, :1]
            neg = self.forward_sdf((x - e).clamp(-bound, bound), bound)[:, :1]
            outs.append(0.5 * (pos - neg) / epsilon)
        return torch.cat(outs, dim=-1)
