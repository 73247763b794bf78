#!/usr/bin/env python3
"""Generate tests/golden/run_long_train.npz: training renders of the reference's own run() at sample counts outside the fused renderer's window,
the ones the long renderer (ac_render_rays_long) and the long compositing backward serve -- made the way make_long_golden.py makes run_long.npz:
the reference imported here, its CUDA back ends stubbed, the hash back end served by oracle/.  The field is nsr_params.npz's
(make_golden.build_reference_net).

    python tests/golden/make_long_train_golden.py [REFERENCE_DIR]

Cases, 32 rays each with recorded jitter noise (keys prefixed "train_<num_steps>_<upsample_steps>/"): (128, 128), (100, 64), (256, 0), (40, 16).
Per case: image, weights_sum, gradient_error, z_vals, and the gradients of  <G, rgb> + 0.01 * gradient_error + <Gw, weight_sum>  (G [32,3], Gw [32] fixed
random) w.r.t. every MLP parameter and the variance ("grad.<name>") and a sample of table rows (emb_idx, emb_grad; emb_max = the largest
magnitude over the whole table gradient).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference and installs the stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.common import make_rays  # noqa: E402

CASES = [(128, 128), (100, 64), (256, 0), (40, 16)]
W_EIK = 0.01
EMB_ROWS = 2048


def run_case(net, ro, rd, bg, G, Gw, num_steps, upsample_steps, seed):
    N = ro.shape[0]
    net.train(True)
    torch.manual_seed(seed)
    noise = torch.rand(N, num_steps).numpy().copy()
    torch.manual_seed(seed)                         # the render draws the same jitter again
    net.zero_grad()
    out = net.render(torch.from_numpy(ro)[None], torch.from_numpy(rd)[None], num_steps=num_steps, bound=1.6, upsample_steps=upsample_steps,
                     staged=False, bg_color=torch.from_numpy(bg), cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0, render_can=True, perturb=True)
    loss = (out["rgb"][0] * torch.from_numpy(G)).sum() + W_EIK * out["gradient_error"] + (out["weight_sum"][:, 0] * torch.from_numpy(Gw)).sum()
    loss.backward()
    res = dict(rays_o=ro, rays_d=rd, bg=bg, noise=noise, G=G, Gw=Gw, w_eik=np.float32(W_EIK),
               image=out["rgb"][0].detach().numpy(), weights_sum=out["weight_sum"][:, 0].detach().numpy(),
               gradient_error=np.float32(out["gradient_error"].item()), z_vals=out["z_vals"].detach().numpy(), num_steps=np.int32(num_steps),
               upsample_steps=np.int32(upsample_steps))
    for k, prm in net.named_parameters():
        if k != "encoder.embeddings":
            res["grad." + k] = prm.grad.numpy().copy()
    ge = net.encoder.embeddings.grad.numpy()
    nz = np.flatnonzero(np.abs(ge).sum(1))
    pick = np.sort(nz[np.random.RandomState(8).choice(len(nz), min(EMB_ROWS, len(nz)), replace=False)])
    res["emb_idx"] = pick.astype(np.int64)
    res["emb_grad"] = ge[pick].copy()
    res["emb_max"] = np.float32(np.abs(ge).max())
    return res


def main():
    net = MG.build_reference_net()
    ro, rd = make_rays(8, 4, dist=1.7, f=4.0, jitter_seed=21)          # 32 rays through the object (run_long.npz's)
    N = ro.shape[0]
    bg = np.random.RandomState(22).uniform(0, 1, size=(N, 3)).astype(np.float32)
    rs = np.random.RandomState(23)
    G = rs.normal(0.0, 1.0, (N, 3)).astype(np.float32)
    Gw = rs.normal(0.0, 1.0, (N,)).astype(np.float32)
    out = {}
    for k, (ns, us) in enumerate(CASES):
        c = run_case(net, ro, rd, bg, G, Gw, ns, us, 41 + k)
        out.update({f"train_{ns}_{us}/{key}": v for key, v in c.items()})
        print(f"train {ns}+{us}: weights_sum", c["weights_sum"].min(), c["weights_sum"].max(), "eik", c["gradient_error"], "emb_max", c["emb_max"])
    np.savez_compressed(os.path.join(HERE, "run_long_train.npz"), **out)


if __name__ == "__main__":
    main()
