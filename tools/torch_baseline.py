"""Stock PyTorch-ROCm (MIOpen/hipBLASLt) ResNet training-step timing: the yardstick our kernels must beat.

Not part of the framework: a measurement tool only.
"""
import argparse, time, json, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from pytorch_distributed_template_amd.models import registry

p = argparse.ArgumentParser()
p.add_argument("--arch", default="resnet18")
p.add_argument("--bs", type=int, default=1200)
p.add_argument("--steps", type=int, default=10)
p.add_argument("--dtype", default="bf16")
p.add_argument("--benchmark", type=int, default=1, help="cudnn.benchmark (MIOpen search) as the reference sets it")
p.add_argument("--cl", type=int, default=1)
p.add_argument("--native-depthwise", default="off", choices=["off", "on"],
               help="on: qualifying depthwise convs run on the native HIP kernels (ops/depthwise.py); off: MIOpen")
p.add_argument("--native-bnact", default="off", choices=["off", "on"],
               help="on: qualifying BatchNorm2d (+ ReLU / ReLU6 / Hardswish) layers run on the native fused HIP kernels "
                    "(ops/bnact.py); off: MIOpen batch norm + a separate activation")
p.add_argument("--native-pointwise", default="off", choices=["off", "on"],
               help="on: qualifying 1x1 convs run on the native HIP kernels (ops/pointwise.py); off: MIOpen")
p.add_argument("--native-stem", default="off", choices=["off", "on"],
               help="on: a qualifying 3x3/2 first conv runs on the native HIP kernels (ops/stemconv.py); off: MIOpen")
p.add_argument("--native-convstats", default="off", choices=["off", "on"],
               help="on (with --native-pointwise on and --native-bnact on): converted 1x1 convs emit the statistics of "
                    "the BatchNorm behind them (ops/convstats.py); off: the BatchNorm reads the conv output for them")
a = p.parse_args()
torch.backends.cudnn.benchmark = bool(a.benchmark)
import threading


def _heartbeat():  # MIOpen's search can stay silent for minutes: keep the run visibly alive
    while True:
        time.sleep(30)
        print("...", flush=True)


threading.Thread(target=_heartbeat, daemon=True).start()
dev = torch.device("cuda:0")
m = registry.create(a.arch).to(dev)
n_dw = 0
if a.native_depthwise == "on":
    from pytorch_distributed_template_amd.ops.depthwise import convert_depthwise
    n_dw = convert_depthwise(m)
    print(f"native depthwise: {n_dw} conv(s) converted", flush=True)
n_pw = 0
if a.native_pointwise == "on":
    from pytorch_distributed_template_amd.ops.pointwise import convert_pointwise
    n_pw = convert_pointwise(m)
    print(f"native pointwise: {n_pw} conv(s) converted", flush=True)
n_stem = 0
if a.native_stem == "on":
    from pytorch_distributed_template_amd.ops.stemconv import convert_stem
    n_stem = convert_stem(m)
    print(f"native stem: {n_stem} conv(s) converted", flush=True)
n_bn = n_act = 0
if a.native_bnact == "on":
    from pytorch_distributed_template_amd.ops.bnact import convert_bnact
    n_bn, n_act = convert_bnact(m)
    print(f"native bnact: {n_bn} BatchNorm(s) converted, {n_act} activation(s) fused", flush=True)
n_cs = 0
if a.native_convstats == "on":
    if a.native_pointwise != "on" or a.native_bnact != "on":
        print("native convstats: ignored, it needs --native-pointwise on and --native-bnact on", flush=True)
    else:
        from pytorch_distributed_template_amd.ops.convstats import convert_convstats
        n_cs = convert_convstats(m)
        print(f"native convstats: {n_cs} conv/BatchNorm pair(s) fused", flush=True)
if a.cl:
    m = m.to(memory_format=torch.channels_last)
opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
crit = nn.CrossEntropyLoss()
x = torch.randn(a.bs, 3, 224, 224, device=dev)
if a.cl:
    x = x.to(memory_format=torch.channels_last)
y = torch.randint(0, 1000, (a.bs,), device=dev)
dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": None}[a.dtype]
def step():
    with torch.autocast("cuda", dtype=dt, enabled=dt is not None):
        out = m(x)
        loss = crit(out, y)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
for i in range(3):  # warm-up (MIOpen's benchmark-mode search happens here: print progress, it can be long)
    t0 = time.time()
    step()
    torch.cuda.synchronize()
    print(f"warm-up step {i}: {time.time() - t0:.1f} s", flush=True)
t = time.time()
for _ in range(a.steps):
    step()
    torch.cuda.synchronize()
    print(".", end="", flush=True)
print()
el = (time.time() - t) / a.steps
print(json.dumps({"arch": a.arch, "bs": a.bs, "dtype": a.dtype, "channels_last": a.cl,
                  "native_depthwise": a.native_depthwise, "depthwise_converted": n_dw,
                  "native_pointwise": a.native_pointwise, "pointwise_converted": n_pw,
                  "native_stem": a.native_stem, "stem_converted": n_stem,
                  "native_bnact": a.native_bnact, "bnact_converted": n_bn, "bnact_fused": n_act,
                  "native_convstats": a.native_convstats, "convstats_pairs": n_cs, "ms_per_step": el * 1e3,
                  "img_per_s": a.bs / el, "max_mem_GB": torch.cuda.max_memory_allocated() / 1e9}))
