#!/usr/bin/env python3
"""Generate tests/golden/warp_render_long.npz: the reference's own run(render_can=False, verts, faces, Ts) at sample counts outside the fused
renderer's window (the long posed renderer, ac_render_rays_long_warped), recorded exactly as make_golden.make_warp_render_golden records
warp_render.npz at 32 + 32 -- the reference imported here, its CUDA back ends stubbed, the hash back end and the libigl stand-in served by oracle/.
The field is nsr_params.npz's (make_golden.build_reference_net), the body tests.common.make_body().

    python tests/golden/make_warp_render_long.py [REFERENCE_DIR]

Cases (keys prefixed "<num_steps>_<upsample_steps>_"): 128 + 128 and 100 + 64, 16 x 16 rays (dist 1.8, f 14, jitter seed 5), mesh guide on, eval mode,
white background.  Data only: rays, background and the reference's outputs.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference and installs the stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.common import make_rays, make_body  # noqa: E402

CASES = [(128, 128), (100, 64)]


def main():
    MG.install_igl_standin()
    verts, faces, Ts = make_body()
    net = MG.build_reference_net()
    net.eval()
    ro, rd = make_rays(16, 16, dist=1.8, f=14.0, jitter_seed=5)
    bg = np.ones((ro.shape[0], 3), np.float32)
    res = {}
    for ns, us in CASES:
        with torch.no_grad():
            out = net.render(torch.from_numpy(ro)[None], torch.from_numpy(rd)[None], num_steps=ns, bound=1.6, upsample_steps=us, staged=False,
                             bg_color=torch.from_numpy(bg), cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0, render_can=False, verts=verts,
                             faces=faces, Ts=Ts, perturb=False, use_mesh_guide=True)
        tag = f"{ns}_{us}"
        res.update({f"{tag}_image": out["rgb"][0].numpy(), f"{tag}_weights_sum": out["weight_sum"][:, 0].numpy(), f"{tag}_depth": out["depth"][0].numpy(),
                    f"{tag}_normal_map": out["normal"].numpy(), f"{tag}_weights": out["weights"].numpy(), f"{tag}_alpha": out["pts_alpha"].numpy(),
                    f"{tag}_z_vals": out["z_vals"].numpy(), f"{tag}_gradient_error": np.float32(out["gradient_error"].item())})
        print("warp render", tag, "mean opacity", float(out["weight_sum"].mean()), "rays with opacity > 0.5:", int((out["weight_sum"] > 0.5).sum()))
    np.savez_compressed(os.path.join(HERE, "warp_render_long.npz"), rays_o=ro, rays_d=rd, bg=bg, **res)


if __name__ == "__main__":
    main()
