#!/usr/bin/env python3
"""bench.py -- headline benchmark of the AvatarCraft hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): render_canonical.py 256x256, hash-grid Instant-NSR, 64+64 samples per
ray, eval mode, white background, 16 batches of 4096 rays per image (render_utils.py:514-600).
One STEP = one pass of the hot path (NeRFRenderer.run, here one ac_render_rays launch + the eikonal
reduce) over one 4096-ray batch; step k renders batch k % 16 of the view.  Inputs (rays, 49 MB hash table,
MLP weights) are resident in HBM before the timed region.  value = rays / s over all ranks (weak scaling:
every rank renders its own view, no data-path collective -- rays are independent).

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: nothing else runs on the GPU or the
CPU.  Printed JSON (rank 0, one line) carries the contract fields plus
  roofline     : dominant kernel (render_rays_kernel) against the HBM roofline with the ALGORITHMIC bytes of
                 SURVEY 8(d): 1 032 192 gather bytes per ray (1008 hash evals x 1024 B) x 4096 rays per launch,
                 divided by the mean launch duration measured with HIP events on the launch stream (the timed steps' own).
--full adds everything that takes runs of its own:
  roofline.other_precision, roofline.whole_view_in_one_launch : the same kernel in the other arithmetic mode, and on the whole view
                 in one launch.
  cpu_baseline : the CPU oracle (oracle/, a port of the reference algorithm; OpenMP over rays) timed on this
                 host on a bounded sample of the same workload.  A reported baseline, not the target.
  the further workloads (sds_step, sds_view_fine, posed_frame, viewdirs, mesh_export_512, density_grid_update, occupancy_render,
                 the guidance stand-in, real_sd) and, on N > 1, same_job_solo.  The options that choose or skip
                 them (--sds-steps, --posed-frames, --no-* ...) take effect only with --full.

This file holds the contract: arguments, the timed region of the headline metric, the JSON line.  Every further workload
and the `--gpus N` self-launcher live in bench_legs/, one module each.
"""
import argparse
import json
import os
import sys
import time

ROOT_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT_DIR)

import numpy as np
import torch

from bench_legs.common import BYTES_PER_RAY, FLOP_PER_RAY, H, HBM_PEAK_GBS, NUM_STEPS, RAYS_PER_BATCH, ROOT, UPSAMPLE_STEPS, W, XGMI_LINKS, XGMI_LINK_GBS, make_inputs
from bench_legs.cpu import cpu_baseline, cpu_baseline_sds
from bench_legs.sds import time_sds_fine_view, time_sds_step, time_sds_step_fp32_records
from bench_legs.posed import time_posed_frame
from bench_legs.variants import time_geometry, time_occupancy_render, time_viewdirs
from bench_legs.guidance import time_real_sd_step, time_sd_arch_step
from bench_legs.launch import _flush_c_stdio, self_launch
from bench_legs.common import SAMPLES, SDS_BYTES_LAUNCHED, SDS_BYTES_SURVEY, make_net, oracle_field, sds_view, _binding, _grid_roofline  # noqa: F401  (re-exported: tools/ and tests/ read them here)
from bench_legs.launch import _free_port, _launch_once  # noqa: F401

def measure_solo(dev, p, field, table, ro, rd, rank, a):
    """this rank alone, no process group: rays/s of the headline launches and ms per SDS step (see main)"""
    from avatarcraft_amd import nsr_ops
    ro_t, rd_t = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    nb = (H * W) // RAYS_PER_BATCH
    outs = [dict() for _ in range(nb)]
    inv_s = float(p["inv_s"])

    def step(k):
        b = k % nb
        sl = slice(b * RAYS_PER_BATCH, (b + 1) * RAYS_PER_BATCH)
        nsr_ops.render_rays(field, ro_t[sl], rd_t[sl], NUM_STEPS, UPSAMPLE_STEPS, 1.6, inv_s, out=outs[b], precision=a.precision)
    for k in range(a.warmup):
        step(k)
    best = None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.steps):
            step(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    out = {"rays_per_s": a.steps * RAYS_PER_BATCH / best, "ms_per_step": best / a.steps * 1e3}
    if a.sds_steps > 0:
        try:
            sds, nets = time_sds_step(dev, p, table, rank, 1, None, a.sds_steps)
            del nets
            out["sds_ms_per_step"] = sds["ms_per_step"]
        except Exception as e:                 # noqa: BLE001
            out["sds_error"] = f"{type(e).__name__}: {e}"
    torch.cuda.synchronize()
    return out


def dump_outputs(res, out_dir):
    """every floating-point array of one render_rays result as out_dir/<name>.npy (float32; a few hundred KB for a 4096-ray batch)"""
    os.makedirs(out_dir, exist_ok=True)
    for k, v in sorted(res.items()):
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            np.save(os.path.join(out_dir, f"{k}.npy"), v.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--full", action="store_true", help="after the headline, also measure everything else the line can report: the other precision, the "
                                                        "whole view in one launch, the SDS step, the bench_legs/ workloads, the CPU baselines, the real-SD "
                                                        "probe and, on N > 1, the same-job solo figures (the options below that choose or skip them act "
                                                        "only with --full)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prepared-field", action="store_true", help="A/B: every render workgroup derives the LDS weight layout itself (no ac_field_prepare)")
    ap.add_argument("--precision", choices=["fast", "exact"], default="exact",
                    help="arithmetic of the render kernel (ac_render_opts.precision): exact = the product's default, every product an fp32 fma, GPU == CPU "
                         "oracle bit for bit; fast = opt-in split-bf16 correction for the six finite-difference evaluations + colour network (sample "
                         "positions bit-identical, pixels within 2e-4 of exact)")
    ap.add_argument("--repeat", type=int, default=5, help="number of timed regions of exactly --steps steps each; the headline is the MEDIAN region (all of them are listed)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed regions, write what the last timed step returned (image, weights_sum, depth, normal_map, eik, "
                                                           "eik_res, gradient_error of the 4096-ray batch) as DIR/<name>.npy in float32; rank 0 only")
    ap.add_argument("--sds-steps", type=int, default=8, help="also time this many 4096-ray SDS steps (secondary metric); 0 = skip")
    ap.add_argument("--real-sd", action="store_true", help="time one SDS step with the real Stable-Diffusion guidance if diffusers + the weights are on this "
                                                           "machine (the line's real_sd field says why not otherwise; the probe itself runs in every --full run)")
    ap.add_argument("--sd-arch-steps", type=int, default=2, help="time this many SDS steps with a guidance of Stable-Diffusion 1.5's architecture (random weights: "
                                                                  "what the step costs once the real UNet is in it); 0 = skip")
    ap.add_argument("--no-occupancy", action="store_true", help="skip the occupancy-grid render leg (render(cuda_ray=True): a separate figure beside the headline)")
    ap.add_argument("--no-viewdirs", action="store_true", help="skip the use_viewdirs=True leg (the same render launch and SDS step with view directions)")
    ap.add_argument("--whole-view-backward", action="store_true", help="fine-view leg: also time the whole-view training forward + backward (stylize.WHOLE_VIEW_BACKWARD; ~75 GB of scratch)")
    ap.add_argument("--sd-arch-variants", action="store_true", help="SD-architecture stand-in leg: also time the fp32-preserving PyTorch settings (MIOpen find mode: ~60 s on a fresh box) and the UNet under bf16 autocast")
    ap.add_argument("--no-fp32-records", action="store_true", help="skip the child process that times the SDS step on the full-fp32-record library (sds_step.ms_per_step_fp32_records)")
    ap.add_argument("--no-fine-view", action="store_true", help="skip the fine-stage leg (one optimizer step on a full 256 x 256 view = 16 patches)")
    ap.add_argument("--no-geometry", action="store_true", help="skip the mesh-export (512^3 + marching cubes) and density-grid-update legs")
    ap.add_argument("--posed-frames", type=int, default=4, help="also time this many 256x256 posed-space frames (render_warp.py, secondary metric); 0 = skip")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own (the form the driver uses for N = 1): this process becomes the launcher of N ranks of itself
        raise SystemExit(self_launch(a.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False); the hot path has no CPU fallback")
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch one rank per GPU (python bench.py --gpus N spawns them itself; or "
                         f"python -m torch.distributed.run --nproc-per-node N bench.py --gpus N)")
    backend = os.environ.get("AC_DIST_BACKEND", "nccl")         # "nccl" is RCCL on ROCm; "gloo" lets the N > 1 path be exercised on a 1-GPU box
    if world > torch.cuda.device_count() and backend == "nccl":
        raise SystemExit(f"{world} ranks but {torch.cuda.device_count()} visible GPU(s): RCCL needs one device per rank "
                         f"(AC_DIST_BACKEND=gloo runs the N > 1 code path with ranks sharing a device -- a plumbing check, not a measurement)")
    dev_index = local_rank % torch.cuda.device_count()        # one rank per GPU; more ranks than GPUs only in the gloo plumbing check
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    rccl_ranks = None
    from avatarcraft_amd import nsr_ops
    p, field, table, ro, rd = make_inputs(dev, rank)
    if not a.no_prepared_field:
        field.prepare()                 # the weights in LDS order, once (like NeRFRenderer does per parameter version)
    solo = None
    if world > 1 and a.full:
        # BEFORE the process group exists: what this very GPU does on its own in this very job (the same launches as the timed region below, the same SDS
        # steps without a collective) -- the N = 1 reference of an N > 1 line measured on the same box, clocks and build (`same_job_solo`; the driver
        # computes the scaling efficiency it reports from its own separate N = 1 run)
        solo = measure_solo(dev, p, field, table, ro, rd, rank, a)
    if world > 1 or os.environ.get("AC_BENCH_FORCE_DIST") == "1":      # (forced at world size 1: the RCCL code path of an N > 1 run on a 1-GPU box)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        # an actual collective before anything is timed: the number of ranks that took part in it is what the line reports
        one = torch.ones(1, dtype=torch.float32, device=dev)
        dist.all_reduce(one, op=dist.ReduceOp.SUM)
        torch.cuda.synchronize()
        rccl_ranks = int(round(float(one.item())))
        assert rccl_ranks == dist.get_world_size() == world, (rccl_ranks, dist.get_world_size(), world)

    ro_t, rd_t = torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev)
    inv_s = float(p["inv_s"])
    nb = (H * W) // RAYS_PER_BATCH
    outs = [dict() for _ in range(nb)]           # output buffers allocated once (caller-owned, as in the reference)

    def step(k, ev=None):
        b = k % nb
        sl = slice(b * RAYS_PER_BATCH, (b + 1) * RAYS_PER_BATCH)
        nsr_ops.render_rays(field, ro_t[sl], rd_t[sl], NUM_STEPS, UPSAMPLE_STEPS, 1.6, inv_s, out=outs[b], events=ev, precision=a.precision)

    for k in range(a.warmup):
        step(k)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
    # --repeat timed regions of EXACTLY --steps steps each, every one bracketed by barrier + synchronize on both sides and reduced with MAX over
    # the ranks; the headline is the median region (a single 16 ms region moves by +-1 % from run to run on one box)
    regions = []
    for rep in range(max(1, a.repeat)):
        fence()
        t0 = time.perf_counter()
        for k in range(a.steps):
            step(k, evs[k])
        fence()
        dt_r = time.perf_counter() - t0
        dt_own = dt_r
        if dist is not None:
            tt = torch.tensor([dt_r, -dt_r], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt_r, dt_min = float(tt[0].item()), -float(tt[1].item())
        else:
            dt_min = dt_r
        regions.append((dt_r, dt_min, float(np.mean([s.elapsed_time(e) for s, e in evs]))))
    if a.dump_outputs and rank == 0:
        # what the caller of the timed path received from its last step, before anything below reuses the buffers
        dump_outputs(outs[(a.steps - 1) % nb], a.dump_outputs)
    order = sorted(range(len(regions)), key=lambda i: regions[i][0])
    dt, dt_rank_min, kern_ms = regions[order[len(order) // 2]]
    other = "exact" if a.precision == "fast" else "fast"
    if a.full:
        # the same launches in the OTHER arithmetic mode, outside the timed region (rank 0 reports it next to the headline: `exact` is bit-identical to the
        # CPU oracle, `fast` keeps sample positions / indices / sdf bit-identical and moves pixels by ~1e-6)
        ev2 = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for k in range(min(a.warmup, 2)):
            nsr_ops.render_rays(field, ro_t[:RAYS_PER_BATCH], rd_t[:RAYS_PER_BATCH], NUM_STEPS, UPSAMPLE_STEPS, 1.6, inv_s, out=outs[0], precision=other)
        for k in range(a.steps):
            b = k % nb
            sl = slice(b * RAYS_PER_BATCH, (b + 1) * RAYS_PER_BATCH)
            nsr_ops.render_rays(field, ro_t[sl], rd_t[sl], NUM_STEPS, UPSAMPLE_STEPS, 1.6, inv_s, out=outs[b], events=ev2[k], precision=other)
        torch.cuda.synchronize()
        other_ms = float(np.mean([s.elapsed_time(e) for s, e in ev2]))
        # informational: the same 65 536 rays of the view in ONE launch (the interface takes any ray count; the reference batches by 4096 to bound its
        # memory).  A 4096-ray launch is two rays per wave slot and ends with its slowest pair; sixteen times more rays per launch average that out.
        view_out = {}
        wev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(3)]
        for k in range(4):
            nsr_ops.render_rays(field, ro_t, rd_t, NUM_STEPS, UPSAMPLE_STEPS, 1.6, inv_s, out=view_out, events=wev[k - 1] if k else None, precision=a.precision)
        torch.cuda.synchronize()
        view_ms = float(np.mean([s.elapsed_time(e) for s, e in wev]))
        del view_out

    sds = None
    if a.full and a.sds_steps > 0:
        try:                                   # secondary metric: never let it take the headline line down with it
            sds, _nets = time_sds_step(dev, p, table, rank, world, dist, a.sds_steps)
            del _nets
            if rank == 0 and world == 1 and not a.no_cpu_baseline:
                sds["cpu_baseline"] = cpu_baseline_sds(p, table)
            pt = os.path.join(ROOT, "profiles", "traffic.json")
            if os.path.exists(pt):
                sds["roofline"]["traffic"] = json.load(open(pt)).get("sds_step_hbm_bytes_per_step")
        except Exception as e:                 # noqa: BLE001
            import traceback
            sds = {"error": f"{type(e).__name__}: {e}", "trace": traceback.format_exc()[-600:]}

    if rank == 0:
        total_rays = world * a.steps * RAYS_PER_BATCH
        achieved = BYTES_PER_RAY * RAYS_PER_BATCH / (kern_ms * 1e-3) / 1e9
        traffic = mfma_busy = mfma_src = traffic_note = binding = binding_src = None
        tf = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tf):
            try:
                tj = json.load(open(tf))
                traffic = tj.get("render_rays_kernel_hbm_bytes_per_launch")
                mfma_busy = (tj.get("render_rays_kernel_mfma_busy_frac") or {}).get(a.precision)
                mfma_src = f"profiles/traffic.json (commit {tj.get('commit')}, {tj.get('command')})"
                traffic_note = tj.get("fetch_size_note")
                binding = (tj.get("binding") or {}).get("render_rays_kernel (main bench, 4096 rays)")
                binding_src = tj.get("binding_source") or tj.get("profile")
            except Exception:
                traffic = None
        res = {
            "metric": "rays/sec, 4096-ray batch, 256x256 render (64+64 samples/ray)", "value": total_rays / dt, "unit": "rays/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
            "repeat": len(regions), "ms_per_step_regions": [round(r[0] / a.steps * 1e3, 4) for r in regions],
            "ms_per_step_spread": round((max(r[0] for r in regions) - min(r[0] for r in regions)) / a.steps * 1e3, 4),
            "ms_per_step_rank_min_max": [round(dt_rank_min / a.steps * 1e3, 4), round(dt / a.steps * 1e3, 4)],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "launcher": os.environ.get("AC_BENCH_LAUNCHER", "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else "single process"),
            "dist_backend": (backend if dist is not None else None), "rccl_ranks": rccl_ranks,
            "config": {"workload": "render_canonical 256x256, hash-grid Instant-NSR, 64+64 samples/ray, 16 x 4096-ray batches, eval, 1 view per rank",
                       "rays_per_step": RAYS_PER_BATCH, "table_mb": round(table.nbytes / 1e6, 2), "parallelism": f"dp{world} (independent views, no collective)",
                       "precision": a.precision,
                       "precision_note": ("exact (the product's default and the headline): every product an fp32 fma in the oracle's order, GPU == CPU oracle "
                                          "bit for bit; fast (opt-in): fp32 everywhere except layer 1 of the six finite-difference SDF evaluations (a split-bf16, "
                                          "hi + lo, 3-product correction of the exact fp32 centre evaluation) and the colour network (split-bf16 x 3); sample "
                                          "positions, indices and sdf bit-identical to exact mode, pixels within 4e-6; the other mode's timing is in "
                                          "roofline.other_precision (--full)")},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": "rocprofv3 --pmc FETCH_SIZE pass of this command at the commit named in profiles/traffic.json (not re-measured in this run)",
                         "traffic_note": traffic_note, "kernel": "render_rays_kernel", "kernel_ms": kern_ms,
                         "algorithmic_bytes_per_launch": BYTES_PER_RAY * RAYS_PER_BATCH,
                         # algorithmic FLOP of the two MLPs / kernel time: what a perfect implementation would have to sustain, NOT what the fp32 matrix
                         # pipe did (the offset evaluations' layer 2 runs as vector dot products, the fast mode moves products to bf16 MFMA);
                         # the measured matrix-pipe occupancy is mfma_busy_frac (SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMDs x 256 CUs x kernel clocks), from
                         # the committed PMC pass of this workload: profiles/traffic.json)
                         "algorithmic_tflops": FLOP_PER_RAY * RAYS_PER_BATCH / (kern_ms * 1e-3) / 1e12, "fp32_peak_tflops": 157.3,
                         "mfma_busy_frac": mfma_busy, "mfma_busy_frac_source": mfma_src,
                         # the BINDING resources, counter-derived: `frac` above is a request-byte fraction -- the table lives in L2 / MALL,
                         # HBM itself is at ~0.2 of peak -- what the kernel runs out of is instruction issue and the per-CU gather path; busy fractions of the
                         # committed PMC pass of this workload (tools/collect_profiles.py: busy_objects), not re-measured in this run
                         "issue": (dict(binding["issue"], source=binding_src) if binding and "issue" in binding else None),
                         "gather": (dict(binding["gather"], l2_sector_bytes_per_launch=binding.get("l2_sector_bytes_per_launch"), source=binding_src)
                                    if binding and "gather" in binding else None)},
        }
        if a.full:
            res["roofline"]["other_precision"] = {"precision": other, "kernel_ms": other_ms, "rays_per_s_per_gpu": RAYS_PER_BATCH / (other_ms * 1e-3),
                                                  "frac": BYTES_PER_RAY * RAYS_PER_BATCH / (other_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
            res["roofline"]["whole_view_in_one_launch"] = {"rays": H * W, "kernel_ms": view_ms, "rays_per_s_per_gpu": H * W / (view_ms * 1e-3),
                                                           "frac": BYTES_PER_RAY * H * W / (view_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                           "note": "informational, not the metric's 4096-ray batch"}
        if sds is not None:
            res["sds_step"] = sds
            if world == 1 and not a.no_fp32_records:
                fr = time_sds_step_fp32_records(a.sds_steps)
                sds["ms_per_step_fp32_records"] = fr.get("ms_per_step")
                sds["fp32_records"] = fr
        if a.full:
            # the further workloads of the line (bench_legs/): each in its own try -- a failing leg reports its error in place and the line is still printed --
            # and with its wall time in leg_seconds (what a --full run spends where: VERDICT round 5, What's weak 6)
            leg_s = {}

            def leg(name, fn, trace=500):
                t_leg = time.perf_counter()
                try:
                    out = fn()
                except Exception as e:             # noqa: BLE001
                    import traceback
                    out = {"error": f"{type(e).__name__}: {e}", "trace": traceback.format_exc()[-trace:]}
                leg_s[name] = round(time.perf_counter() - t_leg, 2)
                return out
            if sds is not None and "fp32_records" in sds:
                leg_s["sds_step_fp32_records (child process)"] = sds["fp32_records"].pop("seconds", None)
            if world == 1 and a.posed_frames > 0:
                res["posed_frame"] = leg("posed_frame", lambda: time_posed_frame(dev, p, table, a.posed_frames, cpu=not a.no_cpu_baseline))
            if world == 1 and not a.no_cpu_baseline:
                res["cpu_baseline"] = leg("cpu_baseline", lambda: cpu_baseline(p, table, ro, rd))
            if world == 1 and not a.no_occupancy:
                res["occupancy_render"] = leg("occupancy_render", lambda: time_occupancy_render(dev, p, table, ro_t, rd_t))
            if world == 1 and a.sds_steps > 0 and not a.no_fine_view:
                res["sds_view_fine"] = leg("sds_view_fine", lambda: time_sds_fine_view(dev, p, table, whole_view_backward=a.whole_view_backward), 600)
            if world == 1 and not a.no_viewdirs:
                def _vd():
                    v = time_viewdirs(dev, p, table, ro_t, rd_t)
                    v["render_vs_default"] = v["render_kernel_ms_per_4096_rays"] / kern_ms
                    if sds is not None and "error" not in sds:
                        v["sds_step_vs_default"] = v["sds_step_ms"] / sds["ms_per_step"]
                    return v
                res["viewdirs"] = leg("viewdirs", _vd, 600)
            if world == 1 and not a.no_geometry:
                g = leg("geometry", lambda: time_geometry(dev, p, table), 600)
                res.update(g if "error" not in g else {"mesh_export_512": g})
            if world == 1 and a.sd_arch_steps > 0:
                res["sds_step_sd_arch_standin"] = leg("sds_step_sd_arch_standin", lambda: time_sd_arch_step(dev, p, table, a.sd_arch_steps, variants=a.sd_arch_variants))
            res["leg_seconds"] = leg_s
            try:
                from avatarcraft_amd.guidance import real_sd_probe
                ok_sd, why_sd = real_sd_probe("1.5")
                res["real_sd"] = (time_real_sd_step(dev, p, table) if (ok_sd and a.real_sd) else
                                  (f"available ({why_sd}); pass --real-sd to time it" if ok_sd else f"absent: {why_sd}"))
            except Exception as e:                 # noqa: BLE001
                res["real_sd"] = f"error: {type(e).__name__}: {e}"
        res["hsa_ipc_mode_legacy"] = {"value": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
                                      "set_by": os.environ.get("AC_BENCH_IPC_NOTE", "the environment of this process (not bench.py's launcher)")}
        if solo is not None:
            # informational: rank 0's own solo figures from the same job (the driver derives its efficiency from its own N = 1 run, not from this)
            res["same_job_solo"] = dict(solo, value_over_n_times_solo=res["value"] / (world * solo["rays_per_s"]),
                                        note="rank 0 alone on its GPU before the process group was formed: same launches, same build, same box")
        if world > 1 and sds is not None and "error" not in sds:
            res["sds_step"]["note"] = ("N > 1: one view per rank, ONE all-reduce of the flat 49 MB gradient (+ 1 guard word) per step, averaged inside the "
                                       "collective on RCCL (ReduceOp.AVG)")
            ar_ms = sds.get("grad_allreduce_ms") or 0.0
            if ar_ms > 0:
                nbytes = sds["grad_allreduce_mb"] * 1e6
                busbw = 2.0 * (world - 1) / world * nbytes / (ar_ms * 1e-3) / 1e9
                res["sds_step"]["allreduce_busbw_gbs"] = busbw           # the ring-equivalent bus bandwidth (nccl-tests' definition)
                res["sds_step"]["allreduce_busbw_peak_gbs"] = XGMI_LINKS * XGMI_LINK_GBS
                res["sds_step"]["allreduce_busbw_frac"] = busbw / (XGMI_LINKS * XGMI_LINK_GBS)
            if solo is not None and solo.get("sds_ms_per_step"):
                res["sds_step"]["same_job_solo_ms_per_step"] = solo["sds_ms_per_step"]
                res["sds_step"]["solo_over_n_rank_step_time"] = solo["sds_ms_per_step"] / sds["ms_per_step"]     # 1.0 = the all-reduce is free
        line = json.dumps(res)
    else:
        line = None
    if dist is not None:
        _flush_c_stdio()                      # every rank: RCCL's banner out of C stdio's buffer now, not at exit (after rank 0's line)
        dist.barrier()
        dist.destroy_process_group()
    if line is not None:                      # the JSON line is the last thing the job writes to stdout
        sys.stdout.flush(); sys.stderr.flush()
        _flush_c_stdio()
        print(line, flush=True)


if __name__ == "__main__":
    main()
