#!/usr/bin/env python
"""Per-sample LoRA multipliers: what the rowscale routes cost.  One JSON line per measurement.

  --what kernel  lora_amd_linear_gemm_fwd_rowscale against lora_amd_linear_gemm_fwd at the same tile, and the library
                 route (GEMM + rowdot + rank_update_rowscale), per SD1.5 shape at batch 8 (us per call, hipGraph-timed);
                 the NCHW conv up-projection with the multiplier inside (conv_up_fwd_rowscale) against a separate pass
                 over T followed by conv_up_fwd
  --what unet    no-grad SD1.5 stand-in UNet forward at 512^2, bf16, batch 8 (CFG over 4 settings), reference-default
                 injection rank 4: (a) one scale for the batch (today's routes), (b) four per-sample alphas in one call,
                 (c) four sequential batch-2 calls with tune_lora_scale (ms per batch of 8)
  --what trace   (b) alone, a few calls: the run to put under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lora_amd as L  # noqa: E402
from lora_amd import _C, ops  # noqa: E402
from scripts.kbench import timeit  # noqa: E402

DEV = "cuda:0"
# (M at batch 8, K, N): 64x64 / 32x32 / 16x16 / 8x8 latent rows, 77-token text rows, time-embedding rows
SHAPES = [(32768, 320, 320), (32768, 320, 2560), (8192, 640, 640), (8192, 640, 5120), (2048, 1280, 1280),
          (2048, 1280, 10240), (512, 1280, 1280), (616, 768, 320), (616, 768, 640), (616, 768, 1280), (8, 1280, 320),
          (8, 1280, 1280)]


def emit(d):
    print(json.dumps(d), flush=True)


def kernel(args):
    r, nsel = args.rank, 4
    for M, K, N in SHAPES:
        x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
        w = (torch.randn(N, K, device=DEV) * 0.03).to(torch.bfloat16)
        b = torch.zeros(N, device=DEV, dtype=torch.bfloat16)
        down, up = torch.randn(r, K, device=DEV) * 0.2, torch.randn(N, r, device=DEV) * 0.05
        rows = torch.rand(nsel, r, device=DEV)
        rps = max(M // 8, 1)
        row = {"M": M, "K": K, "N": N, "r": r}
        ring_ok = _C.gemm_supported(x, w, N, r)
        if ring_ok:
            row["ring_us"] = timeit(lambda: _C.linear_gemm_fwd(x, w, b, down, up, 0.7, 0))[0] * 1e6
            row["ring_rowscale_us"] = timeit(lambda: _C.linear_gemm_fwd_rowscale(x, w, b, down, up, 0.7, rows, rps, 0))[0] * 1e6
            row["ratio"] = row["ring_rowscale_us"] / row["ring_us"]
        lib_rows = torch.rand(nsel, r, device=DEV)

        def lib():
            y = torch.nn.functional.linear(x, w, b)
            t = _C.rowdot(x, down, _C.FACTOR_RK)
            _C.rank_update_rowscale_(y, t, up, _C.FACTOR_KR, 0.7, lib_rows, rps)

        row["lib_rowscale_us"] = timeit(lib)[0] * 1e6
        row["static_choice"] = "ring" if ops.static_rowscale_choice(M, K, N, ring_ok) == ops.PS_RING else "lib"
        emit(row)
    for B, C, H in ((8, 320, 64), (8, 640, 32), (8, 1280, 16), (8, 1280, 8)):
        y = torch.randn(B, C, H, H, device=DEV).to(torch.bfloat16)
        t = torch.randn(B, r, H, H, device=DEV)
        up = torch.randn(C, r, device=DEV) * 0.05
        rows = torch.rand(nsel, r, device=DEV)
        inside = timeit(lambda: _C.conv_up_fwd_rowscale_(y, t, up, 0.7, rows))[0] * 1e6
        mult = rows[torch.arange(B, device=DEV) % nsel].view(B, r, 1, 1).contiguous()

        def separate():
            t.mul_(mult)
            _C.conv_up_fwd_(y, t, up, 0.7, 0.0, 0, 0)

        emit({"conv_up": [B, C, H, H], "r": r, "rowscale_inside_us": inside, "pass_then_conv_up_us": timeit(separate)[0] * 1e6})


def build(args):
    from bench import build_unet
    from lora_amd import trainer as T

    torch.manual_seed(0)
    unet = build_unet(torch.device(DEV), torch.bfloat16, seed=0)
    unet.to(memory_format=torch.channels_last)
    L.inject_trainable_lora(unet, r=args.rank)
    T.promote_lora_to_fp32(unet)
    for up, _ in L.extract_lora_ups_down(unet):
        up.weight.data.normal_(0, 0.02)
    unet.eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(8, 4, 64, 64, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    t = torch.full((8,), 500, device=DEV)
    ehs = torch.randn(8, 77, 768, device=DEV, generator=g).to(torch.bfloat16)
    return unet, x, t, ehs


def time_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0]


@torch.no_grad()
def unet(args):
    net, x, t, ehs = build(args)
    alphas = [0.25, 0.5, 1.0, 1.5]

    def uniform():
        net(x, t, ehs)

    def sequential():
        for q, a in enumerate(alphas):
            L.tune_lora_scale(net, a)
            idx = [q, q + 4]
            net(x[idx], t[idx], ehs[idx])

    L.tune_lora_scale(net, 1.0)
    a_ms = time_ms(uniform, args.reps)
    c_ms = time_ms(sequential, args.reps)
    L.tune_lora_scale(net, 1.0)
    L.tune_lora_scale_per_sample(net, alphas)
    b_ms = time_ms(uniform, args.reps)
    L.clear_lora_per_sample(net)
    emit({"metric": "SD1.5 stand-in UNet forward, 512^2, bf16, batch 8, no grad (ms, median / best)",
          "a_uniform": a_ms, "b_per_sample_alphas": b_ms, "c_four_batch2_calls": c_ms,
          "b_over_a": b_ms[0] / a_ms[0], "b_over_c": b_ms[0] / c_ms[0]})


@torch.no_grad()
def trace(args):
    net, x, t, ehs = build(args)
    L.tune_lora_scale_per_sample(net, [0.25, 0.5, 1.0, 1.5])
    for _ in range(args.reps):
        net(x, t, ehs)
    torch.cuda.synchronize()
    emit({"trace": "per-sample alphas, batch 8", "calls": args.reps})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["kernel", "unet", "trace"], default="kernel")
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    {"kernel": kernel, "unet": unet, "trace": trace}[a.what](a)
