"""Per-layer timing of the native pointwise-conv kernels (csrc/kernels/pwconv.hip) against MIOpen.

For every distinct qualifying 1x1 layer of ``--arch`` at ``--image-size`` (found by forward hooks on a CPU pass) and
each pass (forward, backward data, weight gradient) it times, alternating within this process,

* native: ``ops.pointwise.pwconv_fwd / pwconv_dgrad / pwconv_wgrad``
* MIOpen: ``F.conv2d`` and its autograd on ``channels_last`` tensors of the same dtype

with device events around windows of repeated calls after a warm-up, and reports microseconds per call for both
arms, the bytes the pass has to move (forward: read x and w, write y; backward data: read dy and w, write dx; weight
gradient: read x and dy, write dw), the native kernel's achieved TB/s and its share of the HBM streaming rate.
``--resources`` adds each pwconv kernel's VGPR / scratch / occupancy figures from the compile-time resource report
(needs hipcc, no GPU).  ``--stats`` times, per layer and the same way, the forward that also forms the BatchNorm
statistics of its output (``pwconv_fwd_stats``) against ``pwconv_fwd`` followed by ``bnact_stats``.

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
import torch
import torch.nn as nn
import torch.nn.functional as F

HBM_TBS = 6.3  # achievable HBM streaming rate of an MI355X the shares are quoted against


def layer_shapes(arch, size):
    """[(H, W, C, K, count)] of the qualifying 1x1 convs, in network order, distinct."""
    from pytorch_distributed_template_amd.models import registry
    from pytorch_distributed_template_amd.ops.pointwise import qualifies
    model = registry.create(arch).eval()
    seen = {}

    def hook(m, inp, out):
        k = (inp[0].shape[2], inp[0].shape[3], m.in_channels, m.out_channels)
        seen[k] = seen.get(k, 0) + 1

    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, nn.Conv2d) and qualifies(m)]
    with torch.no_grad():
        model(torch.zeros(1, 3, size, size))
    for h in hs:
        h.remove()
    return [k + (n,) for k, n in seen.items()]


def pass_bytes(M, C, K, esize=2):
    x, y, w = M * C * esize, M * K * esize, K * C * esize
    return {"fwd": x + w + y, "dgrad": x + w + y, "wgrad": x + y + K * C * 4}


def kernel_resources():
    """{kernel name: VGPRs, AGPRs, scratch bytes/lane, occupancy waves/SIMD, LDS bytes} of every pwconv kernel, from
    ``hipcc -Rpass-analysis=kernel-resource-usage`` with the build's device flags."""
    from pytorch_distributed_template_amd.ops import _build
    hipcc = shutil.which("hipcc") or os.path.join(_build.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-ffp-contract=fast", "-munsafe-fp-atomics",
           "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", f"-I{_build.CSRC}", "--cuda-device-only", "-c",
           os.path.join(_build.CSRC, "kernels", "pwconv.hip"), "-o", os.devnull,
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
    """gemm<bf16, 128 ch x 128 rows, resident 2 K-steps> style name from the mangled template instance."""
    m = re.search(r"(pwconv_\w+?_kernel)I((?:L[ib]\d+E)+)E", sym)
    if not m:
        return sym
    a = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2))]
    dt = "bf16" if a[0] == 0 else "fp16"
    if m.group(1) == "pwconv_gemm_kernel":
        ks = f"weights resident, {a[3]} K-step(s)" if a[3] else "K loop"
        stats = ", BN statistics" if len(a) > 4 and a[4] else ""
        return f"gemm<{dt}, {a[1] * 32} ch x {a[2] * 64} rows, {ks}{stats}>"
    return f"wgrad<{dt}>"


def resources_md(res):
    lines = ["| kernel | VGPRs | AGPRs | scratch B/lane | occupancy waves/SIMD | LDS B/block |", "|---|---|---|---|---|---|"]
    for k in sorted(res):
        v = res[k]
        lines.append(f"| `{k}` | {v.get('vgpr')} | {v.get('agpr')} | {v.get('scratch')} | {v.get('occ')} | {v.get('lds')} |")
    return "\n".join(lines)


def time_pair(fa, fb, min_time, rounds=3):
    """Seconds per call of ``fa`` and ``fb``: warm-up, then ``rounds`` alternating event-timed windows per arm, each
    long enough that an arm's windows add up to ``min_time``; the median window is reported."""
    def window(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n

    ns = []
    for f in (fa, fb):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t = window(f, 5)
        ns.append(max(5, int(min_time / rounds / max(t, 1e-7)) + 1))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, ns[0]))
        tb.append(window(fb, ns[1]))
    return sorted(ta)[rounds // 2], sorted(tb)[rounds // 2]


def stats_table(a, shapes, pw, dev, dt):
    """--stats: per layer, the conv that also forms the statistics of the BatchNorm behind it against the conv followed
    by the BatchNorm's own statistics pass (which reads the conv output again)."""
    from pytorch_distributed_template_amd.ops import native
    rows = []
    print(f"## {a.arch} @ {a.image_size}, batch {a.bs}, {a.dtype}: pwconv_fwd_stats vs pwconv_fwd + bnact_stats\n")
    print("| H_in | C -> K | layers | fused us | pwconv_fwd + bnact_stats us | fused/unfused | saved us x layers | y MB |")
    print("|---|---|---|---|---|---|---|---|")
    for H, W, C, K, n in shapes:
        M = a.bs * H * W
        x = torch.randn(a.bs, H, W, C, device=dev).to(dt)
        w = (torch.randn(K, C, device=dev) * C ** -0.5).to(dt)
        slots = torch.empty(native.C.stat_slots() * K * 2, dtype=torch.float64, device=dev)

        def unfused():
            y = pw.pwconv_fwd(x, w)
            native.C.bnact_stats(y, slots, M, K)

        tf, tu = time_pair(lambda: pw.pwconv_fwd_stats(x, w), unfused, a.min_time)
        rows.append(dict(arch=a.arch, H=H, W=W, C=C, K=K, layers=n, bs=a.bs, dtype=a.dtype, fused_us=tf * 1e6,
                         unfused_us=tu * 1e6))
        print(f"| {H} | {C} -> {K} | {n} | {tf * 1e6:.1f} | {tu * 1e6:.1f} | {tf / tu:.2f} | {(tu - tf) * 1e6 * n:.0f} | "
              f"{M * K * 2 / 1e6:.1f} |", flush=True)
        del x
        torch.cuda.empty_cache()
    tot_f = sum(r["fused_us"] * r["layers"] for r in rows)
    tot_u = sum(r["unfused_us"] * r["layers"] for r in rows)
    print(f"\nall layers: fused {tot_f / 1e3:.2f} ms, unfused {tot_u / 1e3:.2f} ms (fused/unfused {tot_f / tot_u:.2f})")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--arch", default="mobilenet_v2")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--bs", type=int, default=400, help="images per GPU (the reference's per-GPU batch)")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--passes", default="fwd,dgrad,wgrad")
    p.add_argument("--min-time", type=float, default=0.2, help="seconds of timed work per arm, shape and pass")
    p.add_argument("--benchmark", type=int, default=1, help="cudnn.benchmark (MIOpen search), as the reference sets it")
    p.add_argument("--native-only", action="store_true", help="time the native arm alone (A/B of kernel builds)")
    p.add_argument("--list", action="store_true", help="print the layer shapes and the byte counts only (no GPU)")
    p.add_argument("--resources", action="store_true", help="print the compile-time resource table (no GPU)")
    p.add_argument("--stats", action="store_true",
                   help="time the forward with the BatchNorm-statistics epilogue (pwconv_fwd_stats: the GEMM and the "
                        "partial-row fold) against pwconv_fwd followed by bnact_stats (all their launches)")
    p.add_argument("--json", default="", help="also write the rows to this file")
    a = p.parse_args()

    if a.resources:
        print(resources_md(kernel_resources()))
        return 0
    shapes = layer_shapes(a.arch, a.image_size)
    if a.list:
        for H, W, C, K, n in shapes:
            print(f"H={H} W={W} {C}->{K} x{n}  bytes/pass at bs {a.bs}: {pass_bytes(a.bs * H * W, C, K)}")
        return 0
    if not torch.cuda.is_available():
        print("pwconv_bench: no GPU (timings are measured, never estimated)", file=sys.stderr)
        return 2
    from pytorch_distributed_template_amd.ops import pointwise as pw
    dev, dt = torch.device("cuda:0"), {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    torch.backends.cudnn.benchmark = bool(a.benchmark)  # 1: MIOpen searches for its fastest algorithm
    torch.manual_seed(0)
    rows = []
    if a.stats:
        return stats_table(a, shapes, pw, dev, dt)
    print(f"## {a.arch} @ {a.image_size}, batch {a.bs}, {a.dtype}: native pwconv vs MIOpen\n")
    print("| H_in | C -> K | layers | pass | native us | MIOpen us | native/MIOpen | MB moved | native TB/s | share of 6.3 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for H, W, C, K, n in shapes:
        N = a.bs
        M = N * H * W
        x = torch.randn(N, H, W, C, device=dev).to(dt)           # NHWC storage
        dy = torch.randn(N, H, W, K, device=dev).to(dt)
        w = (torch.randn(K, C, device=dev) * C ** -0.5).to(dt)
        wt = w.t().contiguous()
        xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)  # channels_last NCHW views of the same storage
        wn = w.view(K, C, 1, 1)

        def bwd(mask):
            return lambda: torch.ops.aten.convolution_backward(dyn, xn, wn, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                                               mask)
        arms = {
            "fwd": (lambda: pw.pwconv_fwd(x, w), lambda: F.conv2d(xn, wn)),
            "dgrad": (lambda: pw.pwconv_dgrad(dy, w, wt), bwd([True, False, False])),
            "wgrad": (lambda: pw.pwconv_wgrad(x, dy), bwd([False, True, False])),
        }
        nbytes = pass_bytes(M, C, K)
        for ps in a.passes.split(","):
            if a.native_only:
                tn, _ = time_pair(arms[ps][0], arms[ps][0], a.min_time / 2)
                tm = float("nan")  # not measured
            else:
                tn, tm = time_pair(arms[ps][0], arms[ps][1], a.min_time)
            tbs = nbytes[ps] / tn / 1e12
            rows.append(dict(arch=a.arch, H=H, W=W, C=C, K=K, layers=n, bs=N, dtype=a.dtype, pass_=ps,
                             native_us=tn * 1e6, miopen_us=tm * 1e6, bytes=nbytes[ps], native_tbs=tbs))
            print(f"| {H} | {C} -> {K} | {n} | {ps} | {tn * 1e6:.1f} | {tm * 1e6:.1f} | {tn / tm:.2f} | "
                  f"{nbytes[ps] / 1e6:.1f} | {tbs:.2f} | {100 * tbs / HBM_TBS:.0f} % |", flush=True)
        del x, dy, xn, dyn
        torch.cuda.empty_cache()
    # one training step's worth of pointwise time: every layer, all three passes
    tot_n = sum(r["native_us"] * r["layers"] for r in rows)
    tot_m = sum(r["miopen_us"] * r["layers"] for r in rows)
    print(f"\nall layers x passes measured: native {tot_n / 1e3:.2f} ms, MIOpen {tot_m / 1e3:.2f} ms "
          f"(native/MIOpen {tot_n / tot_m:.2f}; nan = not measured)")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
