"""Squeeze-and-excitation per EfficientNet-B0 shape and pass: the native module against the stock one under autocast.

    python tools/se_bench.py                       # the ten efficientnet_b0 SE shapes at batch 128, bf16: one JSON line each
    python tools/se_bench.py --batch 400
    python tools/se_bench.py --resources           # VGPRs / scratch / occupancy / LDS of every kernel, no GPU

Both arms are the same ``SqueezeExcitation(C, S, SiLU, Sigmoid)`` with the same fp32 parameters on a 16-bit
``channels_last`` input that requires a gradient; the stock arm runs under 16-bit autocast as the torch engine runs it.
The arms alternate call by call in one process; times are device events, medians over ``--reps`` calls, in microseconds.
``bytes`` are the passes' minimum traffic (forward 2 reads + 1 write, backward 3 reads + 1 write of the activation).
"""
import argparse
import copy
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# efficientnet_b0 at 224 x 224: (C, H = W, S)
SHAPES = [(32, 112, 8), (96, 56, 4), (144, 56, 6), (144, 28, 6), (240, 28, 10), (240, 14, 10), (480, 14, 20),
          (672, 14, 28), (672, 7, 28), (1152, 7, 48)]


def resources():
    from pytorch_distributed_template_amd.ops import _build
    hipcc = shutil.which("hipcc") or os.path.join(_build.ROCM, "bin", "hipcc")
    src = os.path.join(_build.CSRC, "kernels", "se.hip")
    cmd = [hipcc] + _build.hip_flags() + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                          "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    print("| kernel<template arguments> | VGPRs | scratch B/lane | occupancy waves/SIMD | static LDS B/block |")
    print("|---|---|---|---|---|")
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        m = re.match(r"\S*?(se_\w+?_kernel)I((?:L[ib]\d+E)+)E", blk)
        if not m:
            continue
        v = [re.search(pat + r": (\d+)", blk).group(1) for pat in (
            " VGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")]
        targs = ", ".join(re.findall(r"L[ib](\d+)E", m.group(2)))
        print(f"| {m.group(1)}<{targs}> | " + " | ".join(v) + " |")


def bench(batch, dtype, reps):
    import torch
    import torch.nn as nn
    from pytorch_distributed_template_amd.models.efficient import SqueezeExcitation
    from pytorch_distributed_template_amd.ops import se
    dev = "cuda"
    for C, hw, S in SHAPES:
        torch.manual_seed(C + hw)
        stock = nn.Sequential(SqueezeExcitation(C, S, nn.SiLU, nn.Sigmoid)).to(dev)
        native = copy.deepcopy(stock)
        assert se.convert_se(native) == 1
        x = torch.randn(batch, C, hw, hw, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        gy = torch.randn_like(x)

        def run_stock():
            with torch.autocast("cuda", dtype=dtype):
                return stock(x)

        arms, times = {"stock": run_stock, "native": lambda: native(x)}, {}
        ev = lambda: torch.cuda.Event(enable_timing=True)
        for rep in range(reps + 3):  # three warm-up rounds
            for arm, fn in arms.items():
                x.grad = None
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                y = fn()
                e1.record()
                y.backward(gy)
                e2.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times.setdefault(arm + "_fwd", []).append(e0.elapsed_time(e1) * 1e3)
                    times.setdefault(arm + "_bwd", []).append(e1.elapsed_time(e2) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        act = x.numel() * x.element_size()
        rec = dict(C=C, HW=hw * hw, S=S, B=batch, dtype=str(dtype).split(".")[1],
                   **{k + "_us": round(v, 1) for k, v in med.items()},
                   fwd_stock_over_native=round(med["stock_fwd"] / med["native_fwd"], 2),
                   bwd_stock_over_native=round(med["stock_bwd"] / med["native_bwd"], 2),
                   native_fwd_TBps=round(3 * act / med["native_fwd"] * 1e-6, 2),
                   native_bwd_TBps=round(4 * act / med["native_bwd"] * 1e-6, 2))
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true", help="the kernels' resource table (needs hipcc, no GPU)")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.resources:
        resources()
        return
    import torch
    bench(a.batch, {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype], a.reps)


if __name__ == "__main__":
    main()
