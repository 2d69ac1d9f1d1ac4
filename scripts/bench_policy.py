#!/usr/bin/env python
"""The price of the reference's precision policy: the BASELINE configs[1] step (SD1.5 UNet, rank-4 LoRA, batch 4, bf16,
channels-last, head-padded projections, hipGraph replay — what bench.py times) three ways in ONE process:

  resident      the default: frozen weights resident in bf16, bf16 latents
  fp32_shadow   --frozen_dtype fp32 with MASTER_MERGE=0: f32-resident weights under bf16 autocast, the in-step merge
                reads cached bf16 shadows of the masters
  fp32_master   --frozen_dtype fp32: the in-step merge reads the f32 masters (no shadows of the adapted weights)

For each: steps/s over --steps timed steps after --warmup, and memory: what was allocated when the leg began (a leg that
starts above the first one's baseline carries leftovers of the leg before it), torch.cuda.max_memory_allocated from the
capture to the last step (the resident model included, its build's staging copy not) and the difference of the two — the
leg's own peak.  Compare the legs within one call only
(boxes differ by 15-20 %).  Prints one JSON line; --out also writes it to a file."""
import argparse
import gc
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import lora_amd as L  # noqa: E402
from lora_amd import _C, ops  # noqa: E402
from lora_amd import trainer as T  # noqa: E402
from lora_amd.standin import DDPMScheduler  # noqa: E402


def leg(name, frozen_fp32, master, args):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    ops.MASTER_MERGE = master
    cdt = torch.bfloat16
    unet = bench.build_unet(dev, torch.float32 if frozen_fp32 else cdt, seed=0)
    unet.to(memory_format=torch.channels_last)
    L.inject_trainable_lora(unet, r=args.rank)
    T.promote_lora_to_fp32(unet)
    unet.train()
    state = T.FlatLoraState([{"params": T.lora_params(unet), "lr": 1e-4, "weight_decay": 1e-2}], max_grad_norm=1.0, device=dev)
    state.attach_direct_grads(unet)
    merged = state.enable_merged_weights(unet)
    sched = DDPMScheduler()
    cfg = T.StepConfig(autocast_dtype=cdt if frozen_fp32 else None)
    g = torch.Generator(device=dev).manual_seed(1234)
    latents = (torch.randn(args.batch, 4, 64, 64, device=dev, generator=g) * 0.18215).to(cdt)
    latents = latents.contiguous(memory_format=torch.channels_last)
    ehs = torch.randn(args.batch, 77, 768, device=dev, generator=g).to(cdt)

    def fwd_bwd(lat, cond):
        return T.forward_backward(unet, sched, lat, cond, cfg, merged=merged)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()   # the build's f32 staging copy is not the step's memory
    runner = T.GraphedForwardBackward(fwd_bwd, latents, ehs, state) if args.mode == "graph" else fwd_bwd

    def step():
        loss = runner(latents, ehs)
        state.step(state.all_reduce())
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = {"leg": name, "steps_per_s": round(args.steps / dt, 3), "loss": round(float(loss), 6),
           "allocated_at_start_GB": round(base / 1e9, 3),
           "max_memory_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3),
           "peak_above_start_GB": round((torch.cuda.max_memory_allocated() - base) / 1e9, 3),
           "master_sites": merged.n_master_sites, "merge_MB": round(merged.bytes_algorithmic / 1e6, 1)}
    print("[bench_policy]", json.dumps(rec), file=sys.stderr, flush=True)
    for m in unet.modules():
        m.__dict__.pop("_grad_sink", None)
        m.__dict__.pop("_merged", None)
    del runner, merged, state, unet, fwd_bwd, step
    T._CKPT_CAND.clear()          # trainer's per-model cache of checkpointing candidates holds the model's modules
    _C.invalidate_weight_caches()
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--mode", choices=["graph", "eager"], default="graph")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_policy.py needs a GPU"
    os.environ.setdefault("LORA_AMD_HEAD_PAD", "1")
    bench.private_miopen_db()
    torch.backends.cudnn.benchmark = True
    for k in ("FWD", "BWD", "WRW"):
        os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + k, "0")
    legs = [leg("resident", False, True, args), leg("fp32_shadow", True, False, args), leg("fp32_master", True, True, args)]
    by = {r["leg"]: r for r in legs}
    rec = {"metric": "steps_per_s of the configs[1] step under three precision policies, one process",
           "device": torch.cuda.get_device_name(0), "mode": args.mode, "batch": args.batch, "rank": args.rank,
           "steps": args.steps, "warmup": args.warmup, "legs": legs,
           "fp32_master_over_resident": round(by["fp32_master"]["steps_per_s"] / by["resident"]["steps_per_s"], 4),
           "fp32_master_over_fp32_shadow": round(by["fp32_master"]["steps_per_s"] / by["fp32_shadow"]["steps_per_s"], 4)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
