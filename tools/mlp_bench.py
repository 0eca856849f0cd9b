"""Per-shape timing of the native GELU-MLP path (ops/mlp.py, csrc/kernels/mlp.hip) against the stock ops.

For every distinct ``Linear -> GELU -> [Dropout] -> Linear`` run of ``--arch`` inside the kernels' contract (found by
forward hooks on a CPU pass) it times, alternating the two arms within this process,

* native: the run's ``nn.Sequential`` after ``ops.mlp.convert_mlp``
* stock:  the same ``nn.Sequential`` unconverted

both under 16-bit autocast on a 16-bit input, forward alone and forward + backward (all five gradients), with device
events around windows of repeated calls after a warm-up.  It reports microseconds per call, the bytes a pass has to move
when the hidden tensor ``[M][Hd]`` is touched as rarely as the native path touches it (forward: read x, write and read
z0, write y, the weights; backward: read dy twice, z0 three times, write and read dz twice, read x, write dx, the
weights and their gradients) and the native arm's share of the HBM streaming rate.  ``--resources`` prints each mlp
kernel's VGPR / scratch / occupancy / LDS figures from the compile-time resource report (needs hipcc, no GPU).

Not part of the framework: a measurement tool only.  Output: a markdown table on stdout, optionally ``--json FILE``.
"""
import argparse
import copy
import json
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn as nn

from pwconv_bench import HBM_TBS, resources_md, time_pair


def run_shapes(arch, size):
    """[(rows per image, C, Hd, Co, count)] of the runs inside the contract, in network order, distinct."""
    from pytorch_distributed_template_amd.models import registry
    from pytorch_distributed_template_amd.ops import mlp
    model = registry.create(arch).eval()
    seen, hooks = {}, []
    for parent in model.modules():
        if type(parent) not in mlp.KINDS:
            continue
        mods = list(parent.children())
        for i in range(len(mods)):
            run = mlp._run_at(mods, i)
            if run:
                def hook(m, inp, out, fc2=run[1]):
                    k = (inp[0].numel() // inp[0].shape[0] // m.in_features, m.in_features, m.out_features, fc2.out_features)
                    seen[k] = seen.get(k, 0) + 1
                hooks.append(run[0].register_forward_hook(hook))
    with torch.no_grad():
        model(torch.zeros(1, 3, size, size))
    for h in hooks:
        h.remove()
    return [k + (n,) for k, n in seen.items()]


def pass_bytes(M, C, Hd, Co, esize=2):
    x, z, y, w = M * C * esize, M * Hd * esize, M * Co * esize, (C + Co) * Hd
    return {"fwd": x + 2 * z + y + w * esize, "fwd+bwd": x + 2 * z + y + w * esize + 2 * y + 3 * z + 2 * z + 2 * x
            + w * (2 * esize + 4)}


def kernel_resources():
    """{kernel name: VGPRs, AGPRs, scratch bytes/lane, occupancy waves/SIMD, LDS bytes} of every mlp kernel, from
    ``hipcc -Rpass-analysis=kernel-resource-usage`` with the build's device flags."""
    from pytorch_distributed_template_amd.ops import _build
    hipcc = shutil.which("hipcc") or os.path.join(_build.ROCM, "bin", "hipcc")
    cmd = [hipcc] + _build.hip_flags() + ["--cuda-device-only", "-c", os.path.join(_build.CSRC, "kernels", "mlp.hip"),
                                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: \S*?(mlp_fc2_\w+?)_kernelI((?:L[ib]\d+E)+)E", line)
        if m:
            a = [int(t) for t in re.findall(r"L[ib](\d+)E", m.group(2))]
            tile = f", {a[1] * 128} ch, BK {a[2]}" if len(a) > 1 else ""
            cur = out.setdefault(f"{m.group(1)}<{'fp16' if a[0] else 'bf16'}{tile}>", {})
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--arch", default="convnext_tiny")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--bs", type=int, default=128, help="images per GPU")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--min-time", type=float, default=0.2, help="seconds of timed work per arm, shape and pass")
    p.add_argument("--list", action="store_true", help="print the run shapes and the byte counts only (no GPU)")
    p.add_argument("--resources", action="store_true", help="print the compile-time resource table (no GPU)")
    p.add_argument("--json", default="", help="also write the rows to this file")
    a = p.parse_args()
    if a.resources:
        print(resources_md(kernel_resources()))
        return 0
    shapes = run_shapes(a.arch, a.image_size)
    if a.list:
        for R, C, Hd, Co, n in shapes:
            print(f"rows/image={R} {C}->{Hd}->{Co} x{n}  bytes/pass at bs {a.bs}: {pass_bytes(a.bs * R, C, Hd, Co)}")
        return 0
    if not torch.cuda.is_available():
        print("mlp_bench: no GPU (timings are measured, never estimated)", file=sys.stderr)
        return 2
    from pytorch_distributed_template_amd.ops import mlp
    dev, dt = torch.device("cuda:0"), {"bf16": torch.bfloat16, "fp16": torch.float16}[a.dtype]
    torch.manual_seed(0)
    rows = []
    print(f"## {a.arch} @ {a.image_size}, batch {a.bs}, {a.dtype}: native MLP run vs the same Sequential unconverted\n")
    print("| rows/image | C -> Hd -> Co | runs | pass | native us | stock us | native/stock | MB moved | native TB/s | "
          "share of 6.3 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for R, C, Hd, Co, n in shapes:
        M = a.bs * R
        stock = nn.Sequential(nn.Sequential(nn.Linear(C, Hd), nn.GELU(), nn.Linear(Hd, Co))).to(dev)
        native = copy.deepcopy(stock)
        assert mlp.convert_mlp(native) == 1
        x = torch.randn(M, C, device=dev).to(dt).requires_grad_(True)
        gy = torch.randn(M, Co, device=dev).to(dt)

        def fwd(m):
            def f():
                with torch.no_grad(), torch.autocast("cuda", dtype=dt):
                    m(x)
            return f

        def both(m):
            def f():
                with torch.autocast("cuda", dtype=dt):
                    y = m(x)
                y.backward(gy)
                x.grad = None
                m.zero_grad(set_to_none=True)
            return f

        nbytes = pass_bytes(M, C, Hd, Co)
        for ps, arm in (("fwd", fwd), ("fwd+bwd", both)):
            tn, ts = time_pair(arm(native), arm(stock), a.min_time)
            tbs = nbytes[ps] / tn / 1e12
            rows.append(dict(arch=a.arch, rows_per_image=R, C=C, Hd=Hd, Co=Co, runs=n, bs=a.bs, dtype=a.dtype, pass_=ps,
                             native_us=tn * 1e6, stock_us=ts * 1e6, bytes=nbytes[ps], native_tbs=tbs))
            print(f"| {R} | {C} -> {Hd} -> {Co} | {n} | {ps} | {tn * 1e6:.1f} | {ts * 1e6:.1f} | {tn / ts:.2f} | "
                  f"{nbytes[ps] / 1e6:.1f} | {tbs:.2f} | {100 * tbs / HBM_TBS:.0f} % |", flush=True)
        del x, gy
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
