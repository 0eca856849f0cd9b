"""Timing of the native 3x3/2 first-conv kernels (csrc/kernels/stem3x3.hip) against MIOpen.

For each output width of ``--k`` and each pass (forward, weight gradient) it times, alternating within this process,

* native:  ``ops.stemconv.stem3x3_fwd / stem3x3_wgrad`` on the fp32 ``channels_last`` image
* library: ``F.conv2d`` / ``aten.convolution_backward`` on ``channels_last`` tensors of the 16-bit dtype, once with the
  fp32 -> 16-bit cast of the image included (what autocast runs every step) and once on an image cast beforehand

by the method of ``tools/pwconv_bench.py``: device events around windows of repeated calls after a warm-up, the arms'
windows alternating, the median window reported.  It prints microseconds per call, the bytes the pass has to move (the
fp32 image, the 16-bit output or dY, the weights), the native kernel's achieved TB/s and its share of the HBM streaming
rate.  ``--resources`` prints each kernel's VGPR / scratch / occupancy / LDS figures from the compile-time resource
report (needs hipcc, no GPU).

Not part of the framework: a measurement tool only.  Output: a markdown table on stdout, optionally ``--json FILE``.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F

from pwconv_bench import HBM_TBS, resources_md


def pass_bytes(N, H, W, K):
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img, out, w = N * H * W * 3 * 4, N * P * Q * K * 2, K * 27
    return {"fwd": img + out + w * 2, "wgrad": img + out + w * 4}


def kernel_resources():
    """{kernel: VGPRs, AGPRs, scratch bytes/lane, occupancy waves/SIMD, LDS bytes} of every stem3x3 kernel, from
    ``hipcc -Rpass-analysis=kernel-resource-usage`` with the build's device flags."""
    from pytorch_distributed_template_amd.ops import _build
    hipcc = shutil.which("hipcc") or os.path.join(_build.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-ffp-contract=fast", "-munsafe-fp-atomics",
           "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", f"-I{_build.CSRC}", "--cuda-device-only", "-c",
           os.path.join(_build.CSRC, "kernels", "stem3x3.hip"), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"] + os.environ.get("PDT_HIP_EXTRA", "").split()
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(demangle(m.group(1)), {})
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def demangle(sym):
    m = re.search(r"(stem3x3_\w+?_kernel)I((?:L[ib]\d+E)+)E", sym)
    if not m:
        return sym
    a = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2))]
    dt = "bf16" if a[0] == 0 else "fp16"
    if m.group(1) == "stem3x3_fwd_kernel":
        return f"fwd<{dt}, {a[1] * 32} ch x {a[2] * 64} pixels>"
    return f"wgrad<{dt}>"


def time_arms(fs, min_time, rounds=3):
    """Seconds per call of every function of ``fs``: warm-up, then ``rounds`` windows per arm, the arms alternating,
    each arm's windows adding up to about ``min_time``; the median window is reported."""
    def window(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    ns = []
    for f in fs:
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        t = window(f, 2)
        ns.append(max(2, int(min_time / rounds / max(t, 1e-7)) + 1))
    ts = [[] for _ in fs]
    for _ in range(rounds):
        for i, f in enumerate(fs):
            ts[i].append(window(f, ns[i]))
    return [sorted(t)[rounds // 2] for t in ts]


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--k", default="16,24,32", help="output widths (channels of the first conv)")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--bs", type=int, default=400, help="images per GPU (the reference's per-GPU batch)")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--passes", default="fwd,wgrad")
    p.add_argument("--min-time", type=float, default=0.2, help="seconds of timed work per arm, width and pass")
    p.add_argument("--benchmark", type=int, default=0, help="cudnn.benchmark (MIOpen search)")
    p.add_argument("--native-only", action="store_true", help="time the native arm alone (A/B of kernel builds)")
    p.add_argument("--resources", action="store_true", help="print the compile-time resource table (no GPU)")
    p.add_argument("--json", default="", help="also write the rows to this file")
    a = p.parse_args()

    if a.resources:
        print(resources_md(kernel_resources()))
        return 0
    if not torch.cuda.is_available():
        print("stem3x3_bench: no GPU (timings are measured, never estimated)", file=sys.stderr)
        return 2
    from pytorch_distributed_template_amd.ops import stemconv as st
    dev, dt = torch.device("cuda:0"), {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    torch.backends.cudnn.benchmark = bool(a.benchmark)
    torch.manual_seed(0)
    N, H, W = a.bs, a.image_size, a.image_size
    P, Q = st.out_hw(H, W)
    x = torch.randn(N, H, W, 3, device=dev)      # NHWC storage, fp32
    xn = x.permute(0, 3, 1, 2)                   # the channels_last NCHW view the torch engine holds
    x16n = xn.to(dt)                             # channels_last, cast beforehand
    assert x16n.is_contiguous(memory_format=torch.channels_last)
    rows = []
    print(f"## 3x3/2 first conv @ {H}x{W}, batch {N}, {a.dtype}, cudnn.benchmark = {a.benchmark}: native vs MIOpen\n")
    print("| K | pass | native us | MIOpen us (cast included) | MIOpen us (image cast beforehand) | native / MIOpen with cast | "
          "MB moved | native TB/s | share of 6.3 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for K in [int(v) for v in a.k.split(",")]:
        w = (torch.randn(K, 3, 3, 3, device=dev) * 27 ** -0.5).to(dt)  # KRSC
        wn = w.permute(0, 3, 1, 2)                                      # (K, C, R, S) view, channels_last
        dy = torch.randn(N, P, Q, K, device=dev).to(dt)
        dyn = dy.permute(0, 3, 1, 2)

        def bwd(img):
            return torch.ops.aten.convolution_backward(dyn, img, wn, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1,
                                                       [False, True, False])
        arms = {
            "fwd": (lambda: st.stem3x3_fwd(x, w), lambda: F.conv2d(xn.to(dt), wn, None, 2, 1),
                    lambda: F.conv2d(x16n, wn, None, 2, 1)),
            "wgrad": (lambda: st.stem3x3_wgrad(x, dy), lambda: bwd(xn.to(dt)), lambda: bwd(x16n)),
        }
        nbytes = pass_bytes(N, H, W, K)
        for ps in a.passes.split(","):
            if a.native_only:
                tn = time_arms(arms[ps][:1], a.min_time)[0]
                tc = tm = float("nan")  # not measured
            else:
                tn, tc, tm = time_arms(arms[ps], a.min_time)
            tbs = nbytes[ps] / tn / 1e12
            rows.append(dict(K=K, H=H, W=W, bs=N, dtype=a.dtype, pass_=ps, native_us=tn * 1e6, miopen_cast_us=tc * 1e6,
                             miopen_us=tm * 1e6, bytes=nbytes[ps], native_tbs=tbs))
            print(f"| {K} | {ps} | {tn * 1e6:.1f} | {tc * 1e6:.1f} | {tm * 1e6:.1f} | {tn / tc:.2f} | "
                  f"{nbytes[ps] / 1e6:.1f} | {tbs:.2f} | {100 * tbs / HBM_TBS:.0f} % |", flush=True)
        del dy, dyn
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
