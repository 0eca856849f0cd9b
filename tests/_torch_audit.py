"""Teacher-forced audit of one torch-engine training step with the four native conversions on (a plain module, not a
conftest): the counterpart of tests/_step_audit.py for ``StemConv2d``, ``PointwiseConv2d``, ``DepthwiseConv2d`` and
``BNAct2d`` (pytorch_distributed_template_amd/ops).

What it reads:

* the ``Tape`` (tests/_tape.py) of one ``TorchTrainer.train_step``: the ops modules read ``native.C.<name>`` at call
  time, so ``monkeypatch.setattr(native, "C", Tape(native.C))`` records every launch of the step;
* the model and ``snapshot(model)`` taken BEFORE the step (the step ends with the optimizer update: the weights the
  forward used are the snapshot's, not the live ones);
* ``Hooks(model)``: for every converted module its input and output (forward hook) and the gradients autograd delivered
  to it and received from it (FULL backward hook: a tensor hook on a block's input would see the sum over the residual
  branch, not the module's own dx).  The tensors are kept by reference, so addresses can be compared.

Two kinds of judgement, both for every converted module:

*Per launch, per element.*  Every recorded launch is judged against fp64 computed from its OWN recorded operands
(``Tape.value_at``), so errors do not compound and the kernels' derived bounds (tests/_numerics.py,
tests/_bnact_numerics.py) apply unchanged:

* pwconv_fwd / pwconv_dgrad / stem3x3_fwd: ``assert_conv`` with n = C, K, 27 (the stem reference is made of
  ``x.to(dtype)``, the value the kernel forms in registers);
* dwconv_fwd / dwconv_dgrad: fp64 grouped ``F.conv2d`` / ``conv2d_input`` with ``conv_bound``, n = R * S;
* the three weight gradients: the ``wgrad_reduce`` output, ``assert_conv`` with dtype float32 and n = M; the two MFMA
  ones (pointwise, stem) over ``conv_wgrad_nominal_mag``, which equals the plain magnitude except for fp16 subnormal
  operands (unscaled fp16 gradients); dwconv.hip uses no MFMA: plain magnitude;
* bnact_stats: the slot totals with ``assert_sum`` and ``n_chain(rows, blocks, lanes)`` from the launcher's return value;
* bn_finalize_slots: its ``sums`` against the recorded slots (fp64 additions of S slots in another order: S * 2**-53 <
  2**-45 of sum|slot|), then ``check_finalize`` from those sums, the module's own eps / momentum and the buffer snapshot
  (the unbiased running variance included);
* bnact_fwd, bnact_bwd_reduce (+ bn_slot_sum), bn_bwd_finalize, bnact_bwd_apply: ``assert_fwd``, the bound of
  ``assert_bwd_sums``, ``check_bwd_finalize`` and the bound of ``assert_bwd_apply`` with the module's ``act``.
* An element whose fp64 pre-activation lies within 8u * mag_u of a breakpoint (``near_breakpoint``) may take either
  branch of act' in fp32.  It is left out of the element comparison of dx; in the backward sums the kernel's term may
  then be anything between -D|g| and D|g| (D = max|act'|: 1, hardswish 1.5), so it enters the sums' bounds with its whole
  magnitude |dz_ref| + D|g| (times |xhat| for the second sum).  Such elements may be at most ``MASK_CAP`` of a tensor.
  The forward needs no mask: every ``act`` is continuous, ``assert_fwd``'s bound holds on either branch.

*Binding, bit for bit* -- what no kernel test can see:

* the activation a launch read IS the module's input storage (same address: no hidden copy) and its output the storage
  the module returned;
* the 16-bit weight operand equals the SNAPSHOT master rounded to the dtype and placed in the kernel's layout by the index
  formulas written out below from logical OIHW (``[K, C]``, its transpose ``[C, K]`` for the data gradient, taps-major
  ``[R, S, C]``, KRSC), not by the ops' permute chains; in a second step the snapshot is the updated master, so a stale
  operand shows;
* the gy a backward launch read is the gradient autograd delivered, rounded to the dtype, NHWC-dense; dx is what the
  module handed back;
* ``p.grad`` of every converted conv equals the ``wgrad_reduce`` output re-laid to OIHW by the formulas below, ``weight.grad``
  / ``bias.grad`` of every BNAct2d equal the recorded dgamma / dbeta, and they are still the FlatParams views;
* running_mean / running_var are the finalize launch's outputs, ``num_batches_tracked`` moved by one;
* every converted module launched each of its kernels exactly once (no fallback).

Completeness (``finish``): every taped launch judged, every parameter gradient and buffer of a converted module judged,
no audited gradient tensor all zero.  Stock modules in between (classifier, pools, adds, squeeze-excitation) are not
judged.
"""
import torch
import torch.nn.functional as F

import _bnact_numerics as bm
import _numerics as nm
from _numerics import U
from _step_audit import MASK_CAP, Finding, report  # noqa: F401  (report: re-exported for the tests)

INF = float("inf")
OUT_OF_SCOPE = ("sgd",)  # the optimizer update that ends TorchTrainer.train_step: not a converted module's launch


def classes():
    from pytorch_distributed_template_amd.ops import bnact, depthwise, pointwise, stemconv
    return stemconv.StemConv2d, pointwise.PointwiseConv2d, depthwise.DepthwiseConv2d, bnact.BNAct2d


def converted(model):
    """[(module path, module)] of the converted modules, in registration order."""
    cls = classes()
    return [(n, m) for n, m in model.named_modules() if isinstance(m, cls)]


def snapshot(model):
    """(parameters, buffers) by name, cloned: what the coming step's forward reads."""
    return ({n: p.detach().clone() for n, p in model.named_parameters()},
            {n: b.detach().clone() for n, b in model.named_buffers()})


class Hooks:
    """What every converted module saw in one step: ``io[path] = dict(x, y, gy, gx, nf, nb)`` (tensors by reference;
    ``nf`` / ``nb``: how often the forward / the backward hook fired)."""

    def __init__(self, model):
        self.io = {}
        self.handles = []
        for path, m in converted(model):
            self.handles.append(m.register_forward_hook(lambda mod, inp, out, p=path: self._fwd(p, inp, out)))
            self.handles.append(m.register_full_backward_hook(lambda mod, gin, gout, p=path: self._bwd(p, gin, gout)))

    def _slot(self, path):
        return self.io.setdefault(path, dict(x=None, y=None, gy=None, gx=None, nf=0, nb=0))

    def _fwd(self, path, inp, out):
        d = self._slot(path)
        d["x"], d["y"], d["nf"] = inp[0], out, d["nf"] + 1

    def _bwd(self, path, gin, gout):
        d = self._slot(path)
        d["gx"], d["gy"], d["nb"] = gin[0], gout[0], d["nb"] + 1

    def clear(self):
        self.io = {}

    def remove(self):
        for h in self.handles:
            h.remove()


# ------------------------------------------------------------------------------- layouts, written out from logical OIHW
def stem_operand(master, dtype):
    """KRSC: op[k, r, s, c] = round16(master[k, c, r, s])."""
    K, C, R, S = master.shape
    m16 = master.to(dtype)
    op = torch.empty(K, R, S, C, dtype=dtype, device=master.device)
    for r in range(R):
        for s in range(S):
            for c in range(C):
                op[:, r, s, c] = m16[:, c, r, s]
    return op


def stem_grad_oihw(dw):
    """KRSC fp32 gradient -> logical [K, C, R, S]: g[k, c, r, s] = dw[k, r, s, c]."""
    K, R, S, C = dw.shape
    g = torch.empty(K, C, R, S, dtype=dw.dtype, device=dw.device)
    for r in range(R):
        for s in range(S):
            for c in range(C):
                g[:, c, r, s] = dw[:, r, s, c]
    return g


def pointwise_operand(master, dtype):
    """[K, C]: op[k, c] = round16(master[k, c, 0, 0])."""
    return master.to(dtype)[:, :, 0, 0].clone()


def pointwise_operand_t(master, dtype):
    """The data gradient's [C, K]: op[c, k] = round16(master[k, c, 0, 0])."""
    K, C = master.shape[:2]
    flat = master.to(dtype).contiguous().view(-1)  # logical OIHW order: element (k, c, 0, 0) at k * C + c
    k = torch.arange(K, device=master.device).view(1, K)
    c = torch.arange(C, device=master.device).view(C, 1)
    return flat[k * C + c]


def depthwise_operand(master, dtype):
    """Taps-major [R, S, C]: op[r, s, c] = round16(master[c, 0, r, s])."""
    C, _, R, S = master.shape
    m16 = master.to(dtype)
    op = torch.empty(R, S, C, dtype=dtype, device=master.device)
    for r in range(R):
        for s in range(S):
            op[r, s, :] = m16[:, 0, r, s]
    return op


def depthwise_oihw(taps):
    """[R, S, C] -> logical [C, 1, R, S]: w[c, 0, r, s] = taps[r, s, c]."""
    R, S, C = taps.shape
    w = torch.empty(C, 1, R, S, dtype=taps.dtype, device=taps.device)
    for r in range(R):
        for s in range(S):
            w[:, 0, r, s] = taps[r, s, :]
    return w


def nhwc16(g, dtype):
    """The gradient a backward launch must read: logical NCHW ``g`` rounded to ``dtype``, NHWC-dense."""
    return g.detach().permute(0, 2, 3, 1).to(dtype).contiguous()


def _same(a, t):
    return torch.is_tensor(a) and torch.is_tensor(t) and a.data_ptr() == t.data_ptr() and a.numel() == t.numel()


def _exact(got, want, name):
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    g, r = got.detach().double().reshape(-1), want.detach().double().reshape(-1)
    bad = (g != r) | torch.isnan(g)
    n = int(bad.sum())
    if n:
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {n} of {g.numel()} elements differ; first element {i}: got {g[i].item()!r}, "
                             f"expected {r[i].item()!r}")
    return 0.0


def _act_dmax(act):
    return 1.5 if act == "hardswish" else 1.0


class Audit:
    """One step's audit: ``run()`` returns the Findings (empty: the step is right).  ``judged``: name -> worst ratio of
    everything judged (``call:<index>``, ``grad:<parameter>``, ``buf:<buffer>``)."""

    def __init__(self, tape, model, io, params_before, buffers_before, dtype, flat=None, family="torch_audit"):
        self.tape, self.model, self.io = tape, model, io
        self.p0, self.b0, self.dtype, self.flat, self.fam = params_before, buffers_before, dtype, flat, family
        self.findings, self.judged, self.nonzero = [], {}, []
        self.S = int(tape.stat_slots())

    # ---------------------------------------------------------------------------------------------- machinery
    def family(self, kind):
        return f"{self.fam}/{kind}"

    def find(self, path, quantity, detail):
        self.findings.append(Finding(path, quantity, INF, detail))

    def judge(self, path, quantity, names, fn):
        try:
            ratio, detail = float(fn() or 0.0), ""
            if ratio > 1.0:
                raise AssertionError(f"ratio {ratio}")
        except AssertionError as e:
            ratio, detail = INF, str(e)
            self.findings.append(Finding(path, quantity, ratio, detail))
        for n in names:
            self.judged[n] = max(self.judged.get(n, 0.0), ratio)

    def one(self, path, name, **match):
        """The single launch ``name`` whose arguments are the tensors given, or None and a finding."""
        if any(not torch.is_tensor(t) for t in match.values()):
            self.find(path, f"{name} launches", "the tensor that identifies the launch was never seen")
            return None
        hits = self.tape.find(name, **match)
        if len(hits) != 1:
            self.find(path, f"{name} launches", f"{len(hits)} launches for this module in the step, expected exactly 1 "
                      "(0: a fallback to stock ops)")
            return None
        return hits[0]

    def val(self, c, k):
        return self.tape.value_at(c.index, c.args[k])

    def want_nonzero(self, path, what, t):
        self.nonzero.append((path, what, t))

    def hooks_of(self, path):
        d = self.io.get(path)
        if d is None or d["nf"] != 1 or d["nb"] != 1:
            self.find(path, "module calls", f"forward / backward hooks fired {d and (d['nf'], d['nb'])} times, expected "
                      "(1, 1)")
            return None
        return d

    def grad_landed(self, path, pname, want, p):
        """``p.grad`` equals ``want`` bit for bit and is still the flat gradient view."""
        def run():
            assert p.grad is not None, f"{pname}: no gradient"
            _exact(p.grad, want, f"{pname}.grad against the recorded launch output")
            if self.flat is not None:
                assert p.grad.data_ptr() == self.flat.grad_flat(p).data_ptr(), f"{pname}.grad left the flat buffer"
            return 0.0
        self.judge(path, f"{pname.rsplit('.', 1)[-1]}.grad landed", [f"grad:{pname}"], run)
        if p.grad is not None:
            self.want_nonzero(path, f"{pname}.grad", p.grad)

    def gy_binding(self, path, c, k, gy, quantity="gy read"):
        def run():
            g = c.args[k]
            assert g.is_contiguous(), "the gradient operand is not NHWC-dense"
            return _exact(self.val(c, k), nhwc16(gy, self.dtype), f"{c.name}: gy against the delivered gradient")
        self.judge(path, quantity, [], run)

    def wgrad_reduced(self, path, c):
        """The wgrad_reduce launch over the workspace of weight-gradient launch ``c``."""
        r = self.one(path, "wgrad_reduce", a0=c.args[2])
        if r is not None and r.index < c.index:
            self.find(path, "wgrad_reduce launches", "the reduction ran before the weight gradient")
            return None
        return r

    # ---------------------------------------------------------------------------------------------- the modules
    def stem(self, path, m, d):
        dt, fam = self.dtype, self.family
        x, y, gy = d["x"], d["y"], d["gy"]
        master = self.p0[f"{path}.weight"]
        K = m.out_channels
        xh = x.detach().permute(0, 2, 3, 1)
        x16 = xh.to(dt)
        f = self.one(path, "stem3x3_fwd", a0=x, a2=y)
        if f is not None:
            w = self.val(f, 1)
            self.judge(path, "16-bit weight operand (KRSC)", [], lambda: _exact(w, stem_operand(master, dt), "stem3x3_fwd: w"))

            def fwd():
                ref, mag = nm.conv_fwd_ref(x16, w, 2, 1)
                return nm.assert_conv(f.outs[2], ref, mag, 27, dt, f"{path}: y", fam("stem3x3_fwd"))
            self.judge(path, "y", [f"call:{f.index}"], fwd)
            self.judge(path, "output storage", [], lambda: _exact(y, f.outs[2].permute(0, 3, 1, 2), f"{path}: returned y"))
        g = self.one(path, "stem3x3_wgrad", a0=x)
        if g is None:
            return
        self.gy_binding(path, g, 1, gy)
        self.want_nonzero(path, "gy", gy)
        r = self.wgrad_reduced(path, g)
        if r is None:
            return
        self.judged[f"call:{g.index}"] = 0.0  # the workspace is judged through its reduction
        dy = self.val(g, 1)
        dw = r.outs[6].view(K, 3, 3, 3)

        def wgrad():
            ref, _ = nm.conv_wgrad_ref(x16, dy, 3, 3, 2, 1)
            mag = nm.conv_wgrad_nominal_mag(x16, dy, 3, 3, 2, 1, dt)
            n = dy.numel() // K
            return nm.assert_conv(dw, ref, mag, n, torch.float32, f"{path}: weight gradient (KRSC)", fam("stem3x3_wgrad"))
        self.judge(path, "weight gradient", [f"call:{r.index}"], wgrad)
        self.grad_landed(path, f"{path}.weight", stem_grad_oihw(dw), m.weight)

    def pointwise(self, path, m, d):
        dt, fam = self.dtype, self.family
        x, y, gy, gx = d["x"], d["y"], d["gy"], d["gx"]
        master = self.p0[f"{path}.weight"]
        K, C = m.out_channels, m.in_channels
        xh = x.detach().permute(0, 2, 3, 1)
        f = self.one(path, "pwconv_fwd", a0=x, a2=y)
        if f is not None:
            w = self.val(f, 1)
            self.judge(path, "16-bit weight operand ([K, C])", [],
                       lambda: _exact(w, pointwise_operand(master, dt), "pwconv_fwd: w"))

            def fwd():
                ref, mag = nm.conv_fwd_ref(xh, w.reshape(K, 1, 1, C), 1, 0)
                return nm.assert_conv(f.outs[2].view(ref.shape), ref, mag, C, dt, f"{path}: y", fam("pwconv_fwd"))
            self.judge(path, "y", [f"call:{f.index}"], fwd)
            self.judge(path, "output storage", [],
                       lambda: _exact(y, f.outs[2].view(xh.shape[:-1] + (K,)).permute(0, 3, 1, 2), f"{path}: returned y"))
        g = self.one(path, "pwconv_wgrad", a0=x)
        if g is None:
            return
        self.gy_binding(path, g, 1, gy)
        self.want_nonzero(path, "gy", gy)
        dy = self.val(g, 1).view(xh.shape[:-1] + (K,))
        b = self.one(path, "pwconv_dgrad", a0=g.args[1])
        if b is not None:
            wt = self.val(b, 1)
            self.judge(path, "16-bit weight operand ([C, K], data gradient)", [],
                       lambda: _exact(wt, pointwise_operand_t(master, dt), "pwconv_dgrad: wt"))

            def dgrad():
                k_ = torch.arange(K, device=wt.device).view(K, 1)
                c_ = torch.arange(C, device=wt.device).view(1, C)
                wk = wt.contiguous().view(-1)[c_ * K + k_].view(K, 1, 1, C)  # wk[k, 0, 0, c] = wt[c, k]
                ref, mag = nm.conv_dgrad_ref(dy, wk, xh.shape[1], xh.shape[2], 1, 0)
                return nm.assert_conv(b.outs[2].view(ref.shape), ref, mag, K, dt, f"{path}: dx", fam("pwconv_dgrad"))
            self.judge(path, "dx", [f"call:{b.index}"], dgrad)
            self.judge(path, "dx handed to autograd", [], lambda: (
                _exact(gx, b.outs[2].view(xh.shape).permute(0, 3, 1, 2), f"{path}: dx against grad_input")))
            self.want_nonzero(path, "dx", b.outs[2])
        r = self.wgrad_reduced(path, g)
        if r is None:
            return
        self.judged[f"call:{g.index}"] = 0.0  # the workspace is judged through its reduction
        dw = r.outs[6].view(K, C)

        def wgrad():
            ref, _ = nm.conv_wgrad_ref(xh, dy, 1, 1, 1, 0)
            mag = nm.conv_wgrad_nominal_mag(xh, dy, 1, 1, 1, 0, dt)
            return nm.assert_conv(dw, ref.reshape(K, C), mag.reshape(K, C), dy.numel() // K, torch.float32,
                                  f"{path}: weight gradient [K, C]", fam("pwconv_wgrad"))
        self.judge(path, "weight gradient", [f"call:{r.index}"], wgrad)
        self.grad_landed(path, f"{path}.weight", dw[:, :, None, None], m.weight)

    def depthwise(self, path, m, d):
        dt, fam = self.dtype, self.family
        x, y, gy, gx = d["x"], d["y"], d["gy"], d["gx"]
        master = self.p0[f"{path}.weight"]
        C, R, st = m.in_channels, m.kernel_size[0], m.stride[0]
        kw = dict(stride=st, padding=R // 2, groups=C)
        x64 = x.detach().double()  # logical NCHW
        f = self.one(path, "dwconv_fwd", a0=x, a2=y)
        if f is not None:
            w = self.val(f, 1)
            self.judge(path, "16-bit weight operand (taps-major [R, S, C])", [],
                       lambda: _exact(w, depthwise_operand(master, dt), "dwconv_fwd: w"))

            def fwd():
                assert (f.args[7], f.args[8]) == (R, st), f"launched with R, stride = {f.args[7:9]}"
                w64 = depthwise_oihw(w).double()
                ref, mag = F.conv2d(x64, w64, **kw), F.conv2d(x64.abs(), w64.abs(), **kw)
                ref, mag = ref.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()
                assert f.outs[2].shape == ref.shape, f"{path}: y shape {tuple(f.outs[2].shape)}"
                return nm.assert_within(f.outs[2], ref, nm.conv_bound(ref, mag, R * R, dt), f"{path}: y", C,
                                        fam("dwconv_fwd"), ref.shape)
            self.judge(path, "y", [f"call:{f.index}"], fwd)
            self.judge(path, "output storage", [], lambda: _exact(y, f.outs[2].permute(0, 3, 1, 2), f"{path}: returned y"))
        g = self.one(path, "dwconv_wgrad", a0=x)
        if g is None:
            return
        self.gy_binding(path, g, 1, gy)
        self.want_nonzero(path, "gy", gy)
        dy64 = self.val(g, 1).double().permute(0, 3, 1, 2)
        b = self.one(path, "dwconv_dgrad", a0=g.args[1])
        if b is not None:
            wb = self.val(b, 1)
            self.judge(path, "16-bit weight operand (taps-major, data gradient)", [],
                       lambda: _exact(wb, depthwise_operand(master, dt), "dwconv_dgrad: w"))

            def dgrad():
                assert (b.args[7], b.args[8]) == (R, st), f"launched with R, stride = {b.args[7:9]}"
                w64 = depthwise_oihw(wb).double()
                ref = torch.nn.grad.conv2d_input(x64.shape, w64, dy64, **kw)
                mag = torch.nn.grad.conv2d_input(x64.shape, w64.abs(), dy64.abs(), **kw)
                ref, mag = ref.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()
                assert b.outs[2].shape == ref.shape, f"{path}: dx shape {tuple(b.outs[2].shape)}"
                return nm.assert_within(b.outs[2], ref, nm.conv_bound(ref, mag, R * R, dt), f"{path}: dx", C,
                                        fam("dwconv_dgrad"), ref.shape)
            self.judge(path, "dx", [f"call:{b.index}"], dgrad)
            self.judge(path, "dx handed to autograd", [],
                       lambda: _exact(gx, b.outs[2].permute(0, 3, 1, 2), f"{path}: dx against grad_input"))
            self.want_nonzero(path, "dx", b.outs[2])
        r = self.wgrad_reduced(path, g)
        if r is None:
            return
        self.judged[f"call:{g.index}"] = 0.0  # the workspace is judged through its reduction
        dw = r.outs[6].view(R, R, C)

        def wgrad():
            assert (g.args[7], g.args[8]) == (R, st), f"launched with R, stride = {g.args[7:9]}"
            ref = torch.nn.grad.conv2d_weight(x64, (C, 1, R, R), dy64, **kw)
            mag = torch.nn.grad.conv2d_weight(x64.abs(), (C, 1, R, R), dy64.abs(), **kw)
            tap = lambda t: torch.stack([torch.stack([t[:, 0, r_, s_] for s_ in range(R)]) for r_ in range(R)])
            n = dy64.numel() // C
            return nm.assert_conv(dw, tap(ref), tap(mag), n, torch.float32, f"{path}: weight gradient [R, S, C]",
                                  fam("dwconv_wgrad"))
        self.judge(path, "weight gradient", [f"call:{r.index}"], wgrad)
        self.grad_landed(path, f"{path}.weight", depthwise_oihw(dw), m.weight)

    def bnact(self, path, m, d):
        dt, fam, S = self.dtype, self.family, self.S
        x, y, gy, gx = d["x"], d["y"], d["gy"], d["gx"]
        C, act = m.num_features, m.act
        a = bm.ACTS.index(act)
        gamma, beta = self.p0[f"{path}.weight"], self.p0[f"{path}.bias"]
        rm0, rv0 = self.b0[f"{path}.running_mean"], self.b0[f"{path}.running_var"]
        xh = x.detach().permute(0, 2, 3, 1)
        x2 = xh.reshape(-1, C)
        rows = x2.shape[0]
        bufs = [f"buf:{path}.running_mean", f"buf:{path}.running_var"]
        # ------------------------------------------------------------------------------------------ forward
        s = self.one(path, "bnact_stats", a0=x)
        fin = None
        if s is not None:
            slots = s.outs[1]
            tot = slots[:S * C * 2].view(S, C, 2).sum(0)

            def stats():
                assert (s.args[2], s.args[3]) == (rows, C), f"launched with rows, C = {s.args[2:4]}"
                blocks, lanes = s.ret
                x64 = x2.double()
                ref = torch.stack([x64.sum(0), (x64 * x64).sum(0)], 1)
                mag = torch.stack([x64.abs().sum(0), (x64 * x64).sum(0)], 1)
                return nm.assert_sum(tot, ref, mag, bm.n_chain(rows, blocks, lanes), f"{path}: sums", 2, fam("bnact_stats"))
            self.judge(path, "statistics sums", [f"call:{s.index}"], stats)
            fin = self.one(path, "bn_finalize_slots", a0=s.args[1])
        coef = None
        if fin is not None:
            coef, sums = fin.outs[8], fin.outs[9]

            def finalize():
                assert fin.args[2].data_ptr() == m.weight.data_ptr() and fin.args[3].data_ptr() == m.bias.data_ptr(), \
                    "gamma / beta are not the module's parameters"
                assert fin.args[6].data_ptr() == m.running_mean.data_ptr() and \
                    fin.args[7].data_ptr() == m.running_var.data_ptr(), "the running statistics are not the module's"
                assert fin.args[10] is True and float(fin.args[1]) == float(rows), fin.args[1]
                tmag = slots[:S * C * 2].view(S, C, 2).abs().sum(0)
                w = nm.assert_within(sums[:2 * C].view(2, C).t(), tot, 2.0 ** -45 * tmag, f"{path}: slot sums", 2,
                                     fam("finalize"))
                ref = nm.bn_finalize_ref(sums[:C], sums[C:2 * C], float(rows), gamma, beta, m.eps, m.momentum, rm0, rv0)
                return max(w, nm.check_finalize(coef, fin.outs[6], fin.outs[7], ref, C, path, fam("finalize")))
            self.judge(path, "coef / running statistics", [f"call:{fin.index}"], finalize)

            def buffers():
                _exact(m.running_mean, fin.outs[6], f"{path}: running_mean against the finalize output")
                _exact(m.running_var, fin.outs[7], f"{path}: running_var against the finalize output")
                return 0.0
            self.judge(path, "running statistics landed", bufs, buffers)
        self.judge(path, "num_batches_tracked", [f"buf:{path}.num_batches_tracked"], lambda: _exact(
            m.num_batches_tracked, self.b0[f"{path}.num_batches_tracked"] + 1, f"{path}: num_batches_tracked"))
        f = self.one(path, "bnact_fwd", a0=x, a2=y)
        if f is not None and fin is not None:
            def fwd():
                assert _same(f.args[1], fin.args[8]), "bnact_fwd did not read this module's coefficients"
                assert f.args[5] == a, f"launched with act {f.args[5]}, the module's is {a} ({act})"
                return bm.assert_fwd(f.outs[2], x2, self.val(f, 1), C, act, dt, f"{path}: out", fam(f"bnact_fwd/{act}"))
            self.judge(path, "out", [f"call:{f.index}"], fwd)
            self.judge(path, "output storage", [], lambda: _exact(y, f.outs[2].permute(0, 3, 1, 2), f"{path}: returned y"))
        # ------------------------------------------------------------------------------------------ backward
        br = self.one(path, "bnact_bwd_reduce", a1=x)
        if br is None or coef is None:
            return
        self.gy_binding(path, br, 0, gy)
        self.want_nonzero(path, "gy", gy)
        g2 = self.val(br, 0).reshape(-1, C)
        cf = self.val(br, 2)
        u, mag_u = bm.u_ref(x2, cf, C)
        unsure = bm.near_breakpoint(u, mag_u, act)
        share = float(unsure.double().mean())
        dz, dzm = bm.dz_ref(g2, x2, cf, C, act)
        ss = self.one(path, "bn_slot_sum", a0=br.args[3])

        def bsums():
            assert _same(br.args[2], fin.args[8]) and br.args[6] == a, "coefficients / act are not this module's"
            assert share <= MASK_CAP, f"{path}: {share:.5f} of the pre-activations are too close to a breakpoint to call"
            blocks, lanes = br.ret
            ref, mag = bm.bwd_reduce_ref(g2, x2, cf, C, act)
            xh_ = nm.bn_xhat(x2, cf, C).abs()
            loose = torch.where(unsure, dz.abs() + _act_dmax(act) * g2.double().abs(), torch.zeros_like(dz))
            extra = torch.stack([loose.sum(0), (loose * xh_).sum(0)], 1)
            bound = (bm.n_chain(rows, blocks, lanes) + 4) * U * mag + extra
            got = br.outs[3][:S * C * 2].view(S, C, 2).sum(0)
            w = nm.assert_within(got, ref, bound, f"{path}: backward sums", 2, fam(f"bnact_bwd_reduce/{act}"))
            if ss is not None:
                smag = br.outs[3][:S * C * 2].view(S, C, 2).abs().sum(0)
                w = max(w, nm.assert_within(ss.outs[3][:2 * C].view(2, C).t(), got, 2.0 ** -45 * smag,
                                            f"{path}: slot sums (backward)", 2, fam("bn_slot_sum")))
            return w
        self.judge(path, "backward sums", [f"call:{br.index}"] + ([f"call:{ss.index}"] if ss is not None else []), bsums)
        bf = self.one(path, "bn_bwd_finalize", a0=ss.args[3]) if ss is not None else None
        if bf is not None:
            def bfin():
                assert _same(bf.args[2], fin.args[8]) and bf.args[3].data_ptr() == m.weight.data_ptr(), \
                    "coefficients / gamma are not this module's"
                assert float(bf.args[1]) == float(rows) and float(bf.args[6]) == 1.0, (bf.args[1], bf.args[6])
                sm = self.val(bf, 0)
                ref = nm.bn_bwd_finalize_ref(sm[:C], sm[C:2 * C], float(rows), self.val(bf, 2), gamma, 1.0, C)
                return nm.check_bwd_finalize(bf.outs[7], bf.outs[4], bf.outs[5], ref, C, path, fam("bwd_finalize"))
            self.judge(path, "dgamma / dbeta / bcoef", [f"call:{bf.index}"], bfin)
            self.grad_landed(path, f"{path}.weight", bf.outs[4], m.weight)
            self.grad_landed(path, f"{path}.bias", bf.outs[5], m.bias)
        ap = self.one(path, "bnact_bwd_apply", a1=x)
        if ap is not None and bf is not None:
            def apply():
                assert _same(ap.args[0], br.args[0]) and _same(ap.args[2], fin.args[8]) and _same(ap.args[3], bf.args[7]) \
                    and ap.args[7] == a, "g / coef / bcoef / act are not this module's"
                assert share <= MASK_CAP, f"{path}: {share:.5f} of the pre-activations are too close to a breakpoint to call"
                ref, mag = bm.bwd_apply_ref(g2, x2, cf, self.val(ap, 3), C, act)
                got = torch.where(unsure, ref, ap.outs[4].reshape(-1, C).double())
                return nm.assert_rounded(got, ref, mag, dt, name=f"{path}: dx", C=C, family=fam(f"bnact_bwd_apply/{act}"))
            self.judge(path, "dx", [f"call:{ap.index}"], apply)
            self.judge(path, "dx handed to autograd", [],
                       lambda: _exact(gx, ap.outs[4].permute(0, 3, 1, 2), f"{path}: dx against grad_input"))
            self.want_nonzero(path, "dx", ap.outs[4])

    # ---------------------------------------------------------------------------------------------- the walk
    def run(self):
        stem_c, pw_c, dw_c, bn_c = classes()
        mods = converted(self.model)
        for path, m in mods:
            d = self.hooks_of(path)
            if d is None:
                continue
            if isinstance(m, stem_c):
                self.stem(path, m, d)
            elif isinstance(m, pw_c):
                self.pointwise(path, m, d)
            elif isinstance(m, dw_c):
                self.depthwise(path, m, d)
            else:
                self.bnact(path, m, d)
        return self.finish(mods)

    def finish(self, mods):
        """Completeness (module docstring)."""
        missing = [f"{c.index}:{c.name}" for c in self.tape.calls
                   if f"call:{c.index}" not in self.judged and c.name not in OUT_OF_SCOPE]
        if missing:
            self.find("tape", "completeness", f"{len(missing)} launches not judged: {missing[:12]}")
        want = []
        for path, m in mods:
            want += [f"grad:{path}.{n}" for n, _ in m.named_parameters(recurse=False)]
            want += [f"buf:{path}.{n}" for n, _ in m.named_buffers(recurse=False)]
        absent = [n for n in want if n not in self.judged]
        if absent:
            self.find("model", "completeness", f"no judgement of: {absent[:12]} ({len(absent)})")
        for path, what, t in self.nonzero:
            if not bool((t != 0).any()):
                self.find(path, f"{what} all zero", "an all-zero gradient leaves its launches judging nothing")
        return self.findings


def audit(tape, model, io, params_before, buffers_before, dtype, flat=None, family="torch_audit"):
    """Findings and the judged table of one recorded step."""
    a = Audit(tape, model, io, params_before, buffers_before, dtype, flat, family)
    found = a.run()
    return found, a.judged
