"""Bandwidth of the BatchNorm elementwise passes (bn_apply / bn_bwd_apply) at ResNet shapes, B = 1200, and of the
four fused BatchNorm + activation passes (bnact_*) at MobileNetV2 shapes, B = 400, against torch's batch_norm +
activation timed alternately in the same process.

    python tools/ew_bench.py [--so A.so B.so ...]   # one subprocess per build of the extension (PDT_NATIVE_SO)
    python tools/ew_bench.py --bnact [--batch 400] [--act relu6]

(Round 5 chose 4 vectors per thread with this script: csrc/kernels/bn.hip kEwU.)

Prints one JSON line per (U, pass, shape): microseconds and TB/s of the bytes the pass must move.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    import torch
    sys.path.insert(0, ROOT)
    from pytorch_distributed_template_amd.ops import native
    C_ = native.C
    dev = "cuda"
    N = 1200
    shapes = [(56, 64), (56, 256), (28, 128), (14, 256), (7, 512), (7, 2048)]
    out = []

    def timeit(fn, reps=10):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    for hw, c in shapes:
        n = N * hw * hw * c
        y = torch.randn(n, device=dev).to(torch.bfloat16)
        r = torch.randn(n, device=dev).to(torch.bfloat16)
        o = torch.empty_like(y)
        o2 = torch.empty_like(y)
        m = torch.empty(n // 8, dtype=torch.uint8, device=dev)
        coef = torch.rand(4 * c, device=dev)
        bc = torch.rand(3 * c, device=dev)
        cases = {
            "apply_relu": (lambda: C_.bn_apply(y, coef, None, None, o, c, 0, True, None), 4),
            "apply_res_relu_mask": (lambda: C_.bn_apply(y, coef, r, None, o, c, 1, True, m), 6.125),
            "apply_bnres_relu_mask": (lambda: C_.bn_apply(y, coef, r, coef, o, c, 2, True, m), 6.125),
            "bwd_apply": (lambda: C_.bn_bwd_apply(y, None, r, bc, o, None, None, None, None, c), 6),
            "bwd_apply_mask_dz": (lambda: C_.bn_bwd_apply(y, m, r, bc, o, None, None, None, o2, c), 8.125),
            "bwd_apply_2br": (lambda: C_.bn_bwd_apply(y, m, r, bc, o, r, bc, o2, None, c), 10.125),
        }
        for name, (fn, bpe) in cases.items():
            us = timeit(fn)
            out.append({"so": os.environ.get("PDT_NATIVE_SO", "in-tree"), "pass": name, "hw": hw, "C": c, "us": round(us, 1),
                        "TB_s": round(bpe * n / us / 1e6, 2)})
            print(json.dumps(out[-1]), flush=True)
        del y, r, o, o2, m


def child_bnact(batch, act):
    """TB/s of the bytes each bnact pass must move (2 bytes per 16-bit element read or written), and torch's
    F.batch_norm + activation forward / backward on the same tensors, the two sides alternating rep by rep."""
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from pytorch_distributed_template_amd.ops import bnact, native
    C_ = native.C
    dev = "cuda"
    a = bnact.ACTS.index(act)
    fn = {"identity": lambda t: t, "relu": F.relu, "relu6": F.relu6, "hardswish": F.hardswish}[act]
    # (H = W, C) of MobileNetV2 BatchNorm inputs at 224 x 224: stem, expanded and depthwise stages, the 1280 head
    shapes = [(112, 32), (112, 96), (56, 144), (28, 192), (14, 384), (14, 576), (7, 960), (7, 1280)]

    def alternate(f_ours, f_torch, reps=10):
        for _ in range(2):
            f_ours(), f_torch()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
        for e in ev:
            e[0].record()
            f_ours()
            e[1].record()
            f_torch()
            e[2].record()
        torch.cuda.synchronize()
        ours = sorted(e[0].elapsed_time(e[1]) for e in ev)[reps // 2] * 1e3
        theirs = sorted(e[1].elapsed_time(e[2]) for e in ev)[reps // 2] * 1e3
        return ours, theirs

    for hw, c in shapes:
        rows = batch * hw * hw
        n = rows * c
        x = torch.randn(rows, c, device=dev).to(torch.bfloat16)
        g = torch.randn(rows, c, device=dev).to(torch.bfloat16)
        o = torch.empty_like(x)
        gamma, beta = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        slots = torch.empty(C_.stat_slots() * c * 2, dtype=torch.float64, device=dev)
        coef = bnact.bnact_stats(x, gamma, beta, rm, rv, 1e-5, 0.1)
        bc = torch.rand(3 * c, device=dev)
        xt = x.view(batch, hw, hw, c).permute(0, 3, 1, 2).detach().requires_grad_(True)  # channels_last NCHW view
        gt = g.view(batch, hw, hw, c).permute(0, 3, 1, 2)
        gam = gamma.clone().requires_grad_(True)
        bet = beta.clone().requires_grad_(True)

        def t_fwd():
            return fn(F.batch_norm(xt, rm, rv, gam, bet, True, 0.1, 1e-5))
        yt = t_fwd()

        def t_bwd():
            torch.autograd.grad(yt, (xt, gam, bet), gt, retain_graph=True)

        def ours_fwd():
            C_.bnact_stats(x, slots, rows, c)
            C_.bnact_fwd(x, coef, o, rows, c, a)

        def ours_bwd():
            C_.bnact_bwd_reduce(g, x, coef, slots, rows, c, a)
            C_.bnact_bwd_apply(g, x, coef, bc, o, rows, c, a)
        passes = {
            "bnact_stats": (lambda: C_.bnact_stats(x, slots, rows, c), 2),
            "bnact_fwd": (lambda: C_.bnact_fwd(x, coef, o, rows, c, a), 4),
            "bnact_bwd_reduce": (lambda: C_.bnact_bwd_reduce(g, x, coef, slots, rows, c, a), 4),
            "bnact_bwd_apply": (lambda: C_.bnact_bwd_apply(g, x, coef, bc, o, rows, c, a), 6),
        }
        for name, (f, bpe) in passes.items():
            us, _ = alternate(f, lambda: None)
            print(json.dumps({"pass": name, "act": act, "B": batch, "hw": hw, "C": c, "us": round(us, 1),
                              "TB_s": round(bpe * n / us / 1e6, 2), "of_6.3": round(bpe * n / us / 1e6 / 6.3, 2)}), flush=True)
        for name, fo, ft in (("forward", ours_fwd, t_fwd), ("backward", ours_bwd, t_bwd)):
            us, ut = alternate(fo, ft)
            print(json.dumps({"pass": name, "act": act, "B": batch, "hw": hw, "C": c, "bnact_us": round(us, 1),
                              "torch_us": round(ut, 1), "torch_over_bnact": round(ut / us, 2)}), flush=True)
        del x, g, o, xt, gt, yt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--so", nargs="+", default=[""])
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--bnact", action="store_true", help="the four bnact passes at MobileNetV2 shapes instead")
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--act", default="relu6", choices=["identity", "relu", "relu6", "hardswish"])
    a = ap.parse_args()
    if a.child:
        child_bnact(a.batch, a.act) if a.bnact else child()
        return
    for so in a.so:
        env = dict(os.environ)
        if so:
            env["PDT_NATIVE_SO"] = so
        extra = ["--bnact", "--batch", str(a.batch), "--act", a.act] if a.bnact else []
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + extra, env=env, timeout=600)
        if r.returncode != 0:
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
