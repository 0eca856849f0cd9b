"""Global attention per ViT shape and pass: the native kernels against what ``F.multi_head_attention_forward`` does.

    python tools/mha_bench.py                      # vit_b_16 / vit_b_32 / vit_l_16 at batch 128, bf16: one JSON line each
    python tools/mha_bench.py --resources          # VGPRs / AGPRs / scratch / occupancy / LDS of every kernel, no GPU

Both arms start from the packed 16-bit in-projection ``[B, N, 3 * heads * 64]`` and end with the token-major ``y`` that
``out_proj`` reads (forward), or with the gradient of the projection (backward).  The stock arm therefore carries the
transposes ``F.multi_head_attention_forward`` makes around its SDPA call: to sequence-first, the split into three
``[B * heads, N, 64]`` operands (viewed ``[B, heads, N, 64]``), and the transpose of the result back.  The arms alternate
call by call in one process; times are device events, medians over ``--reps`` calls, in microseconds.
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

# at 224 x 224: (name, tokens, heads)
SHAPES = [("vit_b_16", 197, 12), ("vit_b_32", 50, 12), ("vit_l_16", 197, 16)]


def resources():
    from pytorch_distributed_template_amd.ops import _build
    hipcc = shutil.which("hipcc") or os.path.join(_build.ROCM, "bin", "hipcc")
    src = os.path.join(_build.CSRC, "kernels", "mha.hip")
    cmd = [hipcc] + _build.hip_flags() + ["--cuda-device-only", "-c", src, "-o", os.devnull,
                                          "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    print("| kernel | VGPRs | AGPRs | scratch B/lane | occupancy waves/SIMD | LDS B/block |")
    print("|---|---|---|---|---|---|")
    for blk in re.split(r"Function Name: ", r.stderr)[1:]:
        m = re.match(r"\S*mha_(fwd|bwd_dq|bwd_dkv)_kernelILi(\d)E", blk)
        if not m:
            continue
        v = [re.search(pat + r": (\d+)", blk).group(1) for pat in (
            " VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]")]
        print(f"| {m.group(1)} {('bf16', 'fp16')[int(m.group(2))]} | " + " | ".join(v) + " |")


def bench(batch, dtype, reps):
    import torch
    import torch.nn.functional as F
    from pytorch_distributed_template_amd.ops import mha
    dev = "cuda"
    for name, N, heads in SHAPES:
        B, E = batch, heads * 64
        torch.manual_seed(N + heads)
        qkv = torch.randn(B, N, 3 * E, device=dev).to(dtype).requires_grad_(True)
        gy = torch.randn(B, N, E, device=dev).to(dtype)

        def stock():  # F.multi_head_attention_forward between in_proj and out_proj, batch_first input
            p = qkv.transpose(0, 1).unflatten(-1, (3, E)).unsqueeze(0).transpose(0, -2).squeeze(-2).contiguous()
            q, k, v = (t.view(N, B * heads, 64).transpose(0, 1).view(B, heads, N, 64) for t in (p[0], p[1], p[2]))
            y = F.scaled_dot_product_attention(q, k, v)
            return y.permute(2, 0, 1, 3).contiguous().view(N, B, E).transpose(0, 1)

        def native():
            return mha._PackedFn.apply(qkv, heads, 64 ** -0.5)

        arms, times = {"stock": stock, "native": native}, {}
        ev = lambda: torch.cuda.Event(enable_timing=True)
        for rep in range(reps + 3):  # three warm-up rounds
            for arm, fn in arms.items():
                qkv.grad = None
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
        rec = dict(shape=name, N=N, heads=heads, B=B, dtype=str(dtype).split(".")[1],
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
