"""Per-layer timing of the native depthwise-conv kernels (csrc/kernels/dwconv.hip, dwconv7.hip) against MIOpen.

For every distinct qualifying depthwise layer of ``--arch`` at ``--image-size`` (found by forward hooks on a CPU pass) and
each pass (forward, backward data, weight gradient) it times, alternating within this process,

* native: ``ops.depthwise.dwconv_fwd / dwconv_dgrad / dwconv_wgrad``; for a 7x7 layer (``--arch convnext_tiny``:
  56x56x96 x3, 28x28x192 x3, 14x14x384 x9, 7x7x768 x3) ``ops.depthwise7.dwconv7_fwd`` with bias ``/ dwconv7_dgrad /
  dwconv7_wgrad`` with the bias gradient
* MIOpen: ``F.conv2d(groups=C)`` (with bias for 7x7) and its autograd on ``channels_last`` tensors of the same dtype

with device events around windows of repeated calls after a warm-up, and reports microseconds per call for both
arms, the bytes the pass has to move (forward / backward data: read one activation, write one; weight gradient: read
two), the native kernel's achieved TB/s and its share of the HBM ceiling.  ``--resources`` prints each dwconv and
dwconv7 kernel's VGPR / scratch / occupancy / LDS figures from the compile-time resource report (needs hipcc, no GPU).

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
    """[(H_in, W_in, C, R, stride, count)] of the qualifying depthwise convs, in network order, distinct."""
    from pytorch_distributed_template_amd.models import registry
    from pytorch_distributed_template_amd.ops.depthwise import qualifies as q35
    from pytorch_distributed_template_amd.ops.depthwise7 import qualifies7
    qualifies = lambda m: q35(m) or qualifies7(m)
    model = registry.create(arch).eval()
    seen = {}

    def hook(m, inp, out):
        k = (inp[0].shape[2], inp[0].shape[3], m.in_channels, m.kernel_size[0], m.stride[0])
        seen[k] = seen.get(k, 0) + 1

    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, nn.Conv2d) and qualifies(m)]
    with torch.no_grad():
        model(torch.zeros(1, 3, size, size))
    for h in hs:
        h.remove()
    return [k + (n,) for k, n in seen.items()]


def pass_bytes(N, H, W, C, st, esize=2):
    P, Q = (H - 1) // st + 1, (W - 1) // st + 1
    big, small = N * H * W * C * esize, N * P * Q * C * esize
    return {"fwd": big + small, "dgrad": big + small, "wgrad": big + small}


def kernel_resources(source="dwconv.hip"):
    """{kernel name: (VGPRs, AGPRs, scratch bytes/lane, occupancy waves/SIMD, LDS bytes)} of every kernel of
    ``source``, from ``hipcc -Rpass-analysis=kernel-resource-usage`` with the build's device flags."""
    from pytorch_distributed_template_amd.ops import _build
    hipcc = shutil.which("hipcc") or os.path.join(_build.ROCM, "bin", "hipcc")
    cmd = [hipcc, f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-ffp-contract=fast", "-munsafe-fp-atomics",
           "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", f"-I{_build.CSRC}", "--cuda-device-only", "-c",
           os.path.join(_build.CSRC, "kernels", source), "-o", os.devnull,
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
    """dwconv_strip_kernel<bf16, 3x3, stride 1, flip> style name from the mangled template instance."""
    m = re.search(r"(dwconv7?_\w+?_kernel)I((?:L[ib]\d+E)+)E", sym)
    if not m:
        return sym
    a = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2))]
    name = m.group(1)
    dt = "bf16" if a[0] == 0 else "fp16"
    if name == "dwconv7_tile_kernel":
        return (f"tile7<{dt}, {a[2]} columns x {a[3]} channel vectors"
                f"{', flipped taps (dgrad)' if a[4] else ''}{', bias' if a[5] else ''}>")
    if name == "dwconv7_wgrad_kernel":
        return f"wgrad7<{dt}>"
    if name == "dwconv_strip_kernel":
        return f"strip<{dt}, {a[1]}x{a[1]}, stride {a[2]}{', flipped taps (dgrad)' if a[3] else ''}>"
    if name == "dwconv_dgrad2_kernel":
        return f"dgrad2<{dt}, {a[1]}x{a[1]}>"
    return f"wgrad<{dt}, {a[1]}x{a[1]}, stride {a[2]}>"


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


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--arch", default="mobilenet_v2")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--bs", type=int, default=400, help="images per GPU (the reference's per-GPU batch)")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--passes", default="fwd,dgrad,wgrad")
    p.add_argument("--min-time", type=float, default=0.3, help="seconds of timed work per arm, shape and pass")
    p.add_argument("--benchmark", type=int, default=1, help="cudnn.benchmark (MIOpen search), as the reference sets it")
    p.add_argument("--native-only", action="store_true", help="time the native arm alone (A/B of kernel builds)")
    p.add_argument("--list", action="store_true", help="print the layer shapes and the byte counts only (no GPU)")
    p.add_argument("--resources", action="store_true", help="print the compile-time resource table (no GPU)")
    p.add_argument("--json", default="", help="also write the rows to this file")
    a = p.parse_args()

    if a.resources:
        print(resources_md({**kernel_resources(), **kernel_resources("dwconv7.hip")}))
        return 0
    shapes = layer_shapes(a.arch, a.image_size)
    if a.list:
        for H, W, C, R, st, n in shapes:
            print(f"H={H} W={W} C={C} {R}x{R}/{st} x{n}  bytes/pass at bs {a.bs}: {pass_bytes(a.bs, H, W, C, st)['fwd']}")
        return 0
    if not torch.cuda.is_available():
        print("dwconv_bench: no GPU (timings are measured, never estimated)", file=sys.stderr)
        return 2
    from pytorch_distributed_template_amd.ops import depthwise as dw, depthwise7 as dw7
    dev, dt = torch.device("cuda:0"), {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    torch.backends.cudnn.benchmark = bool(a.benchmark)  # 1: MIOpen searches for its fastest algorithm
    torch.manual_seed(0)
    rows = []
    print(f"## {a.arch} @ {a.image_size}, batch {a.bs}, {a.dtype}: native dwconv vs MIOpen\n")
    print("| H_in | C | k/stride | layers | pass | native us | MIOpen us | native/MIOpen | MB moved | native TB/s | share of 6.3 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for H, W, C, R, st, n in shapes:
        N = a.bs
        P, Q = (H - 1) // st + 1, (W - 1) // st + 1
        x = torch.randn(N, H, W, C, device=dev).to(dt)           # NHWC storage
        dy = torch.randn(N, P, Q, C, device=dev).to(dt)
        w = (torch.randn(R, R, C, device=dev) / R).to(dt)        # taps-major
        xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)  # channels_last NCHW views of the same storage
        wn = w.permute(2, 0, 1).unsqueeze(1).contiguous()        # [C, 1, R, S]
        kw = dict(stride=st, padding=R // 2, groups=C)
        b = torch.randn(C, device=dev).to(dt) if R == 7 else None  # the 7x7 convs (ConvNeXt) carry a bias
        bwd = lambda mask: torch.ops.aten.convolution_backward(dyn, xn, wn, [C] if R == 7 else None, [st, st],
                                                               [R // 2] * 2, [1, 1], False, [0, 0], C, mask)
        arms7 = {
            "fwd": (lambda: dw7.dwconv7_fwd(x, w, b), lambda: F.conv2d(xn, wn, b, **kw)),
            "dgrad": (lambda: dw7.dwconv7_dgrad(dy, w), lambda: bwd([True, False, False])),
            "wgrad": (lambda: dw7.dwconv7_wgrad(x, dy, True), lambda: bwd([False, True, True])),
        }
        arms = arms7 if R == 7 else {
            "fwd": (lambda: dw.dwconv_fwd(x, w, st), lambda: F.conv2d(xn, wn, **kw)),
            "dgrad": (lambda: dw.dwconv_dgrad(dy, w, H, W, st),
                      lambda: torch.ops.aten.convolution_backward(dyn, xn, wn, None, [st, st], [R // 2] * 2, [1, 1], False,
                                                                  [0, 0], C, [True, False, False])),
            "wgrad": (lambda: dw.dwconv_wgrad(x, dy, R, st),
                      lambda: torch.ops.aten.convolution_backward(dyn, xn, wn, None, [st, st], [R // 2] * 2, [1, 1], False,
                                                                  [0, 0], C, [False, True, False])),
        }
        nbytes = pass_bytes(N, H, W, C, st)
        for ps in a.passes.split(","):
            if a.native_only:
                tn, _ = time_pair(arms[ps][0], arms[ps][0], a.min_time / 2)
                tm = float("nan")  # not measured
            else:
                tn, tm = time_pair(arms[ps][0], arms[ps][1], a.min_time)
            tbs = nbytes[ps] / tn / 1e12
            rows.append(dict(arch=a.arch, H=H, W=W, C=C, R=R, stride=st, layers=n, bs=N, dtype=a.dtype, pass_=ps,
                             native_us=tn * 1e6, miopen_us=tm * 1e6, bytes=nbytes[ps], native_tbs=tbs))
            print(f"| {H} | {C} | {R}x{R}/{st} | {n} | {ps} | {tn * 1e6:.1f} | {tm * 1e6:.1f} | {tn / tm:.2f} | "
                  f"{nbytes[ps] / 1e6:.1f} | {tbs:.2f} | {100 * tbs / HBM_TBS:.0f} % |", flush=True)
        del x, dy, xn, dyn
        torch.cuda.empty_cache()
    # one training step's worth of depthwise time: every layer, all three passes
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
