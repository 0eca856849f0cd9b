"""Window attention per layer shape and pass: the native kernels against the stock SDPA call the modules make.

    python tools/winattn_bench.py                      # swin_t at batch 128, bf16: one JSON line per layer shape
    python tools/winattn_bench.py --resources          # VGPRs / scratch / occupancy / LDS of every kernel, no GPU

Both arms start from the packed 16-bit qkv ``[Bw, N, 3 * heads * 32]`` of the qkv ``Linear`` and the fp32 bias
``[heads, N, N]``, and end with the token-major ``y`` the projection reads (forward), or with the gradients of qkv and
bias (backward).  The stock arm therefore includes what the native path removes: the q / k / v permute, the bias cast,
the shift mask and its ``repeat``, the transpose copy of ``y`` and the reduction of the mask gradient.  The arms
alternate call by call in one process; times are device events, medians over ``--reps`` calls, in microseconds.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# swin_t at 224 x 224: (tokens per side, heads, shifted)
SWIN_T = [(56, 3, False), (56, 3, True), (28, 6, False), (28, 6, True), (14, 12, False), (14, 12, True), (7, 24, False)]


def resources():
    from pytorch_distributed_template_amd.ops import _build
    hipcc = shutil.which("hipcc") or os.path.join(_build.ROCM, "bin", "hipcc")
    src = os.path.join(_build.CSRC, "kernels", "winattn.hip")
    cmd = [hipcc] + _build.hip_flags() + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                          "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    print("| kernel | VGPRs | AGPRs | scratch B/lane | occupancy waves/SIMD | LDS B/block |")
    print("|---|---|---|---|---|---|")
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        m = re.match(r"\S*winattn_(fwd|bwd)_kernelILi(\d)E", blk)
        if not m:
            continue
        v = [re.search(pat + r": (\d+)", blk).group(1) for pat in (
            " VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")]
        print(f"| {m.group(1)} {('bf16', 'fp16')[int(m.group(2))]} | " + " | ".join(v) + " |")


def bench(batch, dtype, reps):
    import torch
    import torch.nn.functional as F
    from pytorch_distributed_template_amd.ops import winattn as wa
    dev, ws, N = "cuda", 7, 49
    for side, heads, shifted in SWIN_T:
        nwin = (side // ws) ** 2
        Bw, C = batch * nwin, heads * 32
        torch.manual_seed(side + heads)
        qkv = torch.randn(Bw, N, 3 * C, device=dev).to(dtype).requires_grad_(True)
        bias = torch.randn(heads, N, N, device=dev).requires_grad_(True)
        gy = torch.randn(Bw, N, C, device=dev).to(dtype)
        region = wa.region_labels(side, side, ws, 3, 3, dev) if shifted else None

        def stock():
            q, k, v = qkv.reshape(Bw, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
            mask = bias.unsqueeze(0).to(dtype)
            if shifted:
                lab = region.to(dtype)
                shift = (lab.unsqueeze(1) - lab.unsqueeze(2)).ne(0).to(dtype) * -100.0
                mask = (mask + shift.unsqueeze(1)).repeat(batch, 1, 1, 1)
            return F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(Bw, N, C)

        def native():
            return wa._PackedFn.apply(qkv, bias, region, heads, 32 ** -0.5)

        arms, times = {"stock": stock, "native": native}, {}
        ev = lambda: torch.cuda.Event(enable_timing=True)
        for rep in range(reps + 3):  # three warm-up rounds
            for name, fn in arms.items():
                qkv.grad = bias.grad = None
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                y = fn()
                e1.record()
                y.backward(gy)
                e2.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times.setdefault(name + "_fwd", []).append(e0.elapsed_time(e1) * 1e3)
                    times.setdefault(name + "_bwd", []).append(e1.elapsed_time(e2) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = dict(side=side, heads=heads, shifted=shifted, Bw=Bw, dtype=str(dtype).split(".")[1],
                   **{k + "_us": round(v, 1) for k, v in med.items()},
                   fwd_stock_over_native=round(med["stock_fwd"] / med["native_fwd"], 2),
                   bwd_stock_over_native=round(med["stock_bwd"] / med["native_bwd"], 2))
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
