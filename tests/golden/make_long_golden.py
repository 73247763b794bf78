#!/usr/bin/env python3
"""Generate tests/golden/run_long.npz: the reference's own run() at sample counts outside the fused renderer's window (the long renderer,
ac_render_rays_long), the same way make_golden.py makes run_*.npz -- the reference imported here, its CUDA back ends stubbed, the hash back end
served by oracle/.  The field is nsr_params.npz's (make_golden.build_reference_net).

    python tests/golden/make_long_golden.py [/root/reference]

Cases, 32 rays each (keys prefixed "<case>/"): eval (128, 128), (100, 64), (256, 0), (96, 32), (40, 16), (16, 496) (31 up-sampling passes,
inv_s up to 64 * 2^30) and one train case (96, 32) with its
recorded jitter noise and the gradients of image.sum() + gradient_error w.r.t. the table (a sample of rows) and the MLP parameters.
RECORDED_FLIPS are the CPU oracle's: the positions (ray, pass, sample) where oracle/'s restatement of run() (whose envelope is the long
renderer's, up to 512 samples) picks a different searchsorted index than the reference, each off by exactly 1.  tests/test_oracle_long.py
asserts that the oracle reproduces exactly these and no others, and that at 16 + 496 its indices differ in no pass the tests compare (the first
five, tests/common.py:LONG_INDEX_PASSES) and in 1 328 over all 31; the GPU tests assert the same of the long renderer, which equals the oracle
bit for bit (tests/test_gpu_long_oracle.py).  They are the kind of ill-conditioned comparison tests/test_oracle_golden.py:_indices_match describes.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference and installs the stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.common import make_rays  # noqa: E402

EVAL_CASES = [(128, 128), (100, 64), (256, 0), (96, 32), (40, 16), (16, 496)]
TRAIN_CASE = (96, 32)
RECORDED_FLIPS = {"eval_128_128": [[9, 5, 10], [9, 6, 11], [18, 4, 9]], "eval_100_64": [[18, 3, 15]]}


def run_long_case(net, ro, rd, num_steps, upsample_steps, train, seed, bg):
    N = ro.shape[0]
    net.train(train)
    noise = None
    if train:
        torch.manual_seed(seed)
        noise = torch.rand(N, num_steps).numpy().copy()
        torch.manual_seed(seed)
    net.zero_grad()
    with MG.Recorder() as rec, torch.set_grad_enabled(train):
        out = net.render(torch.from_numpy(ro)[None], torch.from_numpy(rd)[None], num_steps=num_steps, bound=1.6, upsample_steps=upsample_steps,
                         staged=False, bg_color=torch.from_numpy(bg), cos_anneal_ratio=1.0, normal_epsilon_ratio=0.0, render_can=True, perturb=train)
    nup = upsample_steps // 16
    T = num_steps + upsample_steps
    ss = np.stack([t.numpy() for t in rec.ss], 1).astype(np.int32) if nup else np.zeros((N, 0, 16), np.int32)
    srt = np.full((N, max(nup, 1), T), -1, np.int32)
    for i, t in enumerate(rec.sort):
        srt[:, i, :t.shape[1]] = t.numpy()
    res = dict(rays_o=ro, rays_d=rd, bg=bg, image=out["rgb"][0].detach().numpy(), weights_sum=out["weight_sum"][:, 0].detach().numpy(),
               depth=out["depth"][0].detach().numpy(), normal_map=out["normal"].detach().numpy(), z_vals=out["z_vals"].detach().numpy(),
               gradient_error=np.float32(out["gradient_error"].item()), ss_inds=ss, sort_index=srt,
               oracle_ss_flips=np.array(RECORDED_FLIPS.get(f"{'train' if train else 'eval'}_{num_steps}_{upsample_steps}", []), np.int32).reshape(-1, 3),
               num_steps=np.int32(num_steps), upsample_steps=np.int32(upsample_steps), train=np.int32(train))
    if train:
        res["noise"] = noise
        (out["rgb"][0].sum() + out["gradient_error"]).backward()
        for k, prm in net.named_parameters():
            if k != "encoder.embeddings":
                res["grad." + k] = prm.grad.numpy().copy()
        ge = net.encoder.embeddings.grad.numpy()
        nz = np.flatnonzero(np.abs(ge).sum(1))
        pick = np.sort(nz[np.random.RandomState(8).choice(len(nz), min(4096, len(nz)), replace=False)])
        res["emb_idx"] = pick.astype(np.int64)
        res["emb_grad"] = ge[pick].copy()
        res["emb_max"] = np.float32(np.abs(ge).max())
    return res


def main():
    net = MG.build_reference_net()
    ro, rd = make_rays(8, 4, dist=1.7, f=4.0, jitter_seed=21)          # 32 rays through the object
    bg = np.random.RandomState(22).uniform(0, 1, size=(ro.shape[0], 3)).astype(np.float32)
    out = {}
    for ns, us in EVAL_CASES:
        c = run_long_case(net, ro, rd, ns, us, False, 0, bg)
        out.update({f"eval_{ns}_{us}/{k}": v for k, v in c.items()})
        print(f"eval {ns}+{us}: weights_sum", c["weights_sum"].min(), c["weights_sum"].max(), "eik", c["gradient_error"])
    ns, us = TRAIN_CASE
    c = run_long_case(net, ro, rd, ns, us, True, 31, bg)
    out.update({f"train_{ns}_{us}/{k}": v for k, v in c.items()})
    print(f"train {ns}+{us}: weights_sum", c["weights_sum"].min(), c["weights_sum"].max(), "eik", c["gradient_error"])
    np.savez_compressed(os.path.join(HERE, "run_long.npz"), **out)


if __name__ == "__main__":
    main()
