"""The torch engine's opt-in native ops as two tuples of records, ``TABLE`` (convolutions and normalisations) and, run
after it, ``ATTENTION``: which ``--native-<name>`` flags exist, the order their conversions run in, what each needs and
what it reports.  ``cli.py``, ``engine/runner.py`` and ``tools/torch_baseline.py`` all read
it, so they convert a model the same way.  A new op is one module under ``ops/`` plus one record here."""
from __future__ import annotations

import importlib
from typing import NamedTuple, Tuple


class Conversion(NamedTuple):
    name: str          # flag --native-<name>, dest native_<name>
    help: str          # argparse expands it with %: a literal percent sign is written %%
    module: str        # under ops/, imported only when the flag is on
    function: str      # model -> count, or a tuple of counts
    result: str        # the report, formatted with the counts (positional) and arch=
    needs: Tuple[str, ...] = ()  # conversions that must be on as well
    syncbn_voids: bool = False   # SyncBatchNorm conversion rebuilds every _BatchNorm: nothing of this one would be left


# in the order the conversions run
TABLE = (
    Conversion(
        "depthwise",
        "torch engine: run qualifying depthwise convs (3x3 / 5x5, stride 1 / 2, no bias, channels %% 8 "
        "== 0) on the native HIP depthwise kernels where the activations are 16-bit channels_last "
        "GPU tensors; elsewhere (CPU, fp32, validation) the modules fall back to F.conv2d",
        "depthwise", "convert_depthwise", "{0} conv(s) of {arch} converted"),
    Conversion(
        "pointwise",
        "torch engine: run qualifying 1x1 convs (stride 1, padding 0, groups 1, no bias, both channel "
        "counts %% 8 == 0 and within 8..2048) on the native HIP pointwise kernels where the activations "
        "are 16-bit channels_last GPU tensors; elsewhere (CPU, fp32, validation) the modules fall back "
        "to F.conv2d",
        "pointwise", "convert_pointwise", "{0} conv(s) of {arch} converted"),
    Conversion(
        "stem",
        "torch engine: run a qualifying first conv (3 input channels, 3x3, stride 2, padding 1, no bias, "
        "output channels %% 8 == 0 and within 8..64) on the native HIP stem kernels where the image is an "
        "fp32 channels_last GPU tensor under 16-bit autocast; elsewhere (CPU, fp32, validation) the "
        "module falls back to F.conv2d",
        "stemconv", "convert_stem", "{0} conv(s) of {arch} converted"),
    Conversion(
        "dw7",
        "torch engine: run qualifying 7x7 depthwise convs (stride 1, padding 3, with or without bias, "
        "channels %% 8 == 0: ConvNeXt's block conv) on the native HIP kernels where the activations are "
        "channels_last GPU tensors, 16-bit or fp32 under 16-bit autocast; elsewhere (CPU, fp32 without "
        "autocast, validation) the modules fall back to F.conv2d",
        "depthwise7", "convert_depthwise7", "{0} conv(s) of {arch} converted"),
    Conversion(
        "layernorm",
        "torch engine: run qualifying LayerNorms (one normalised dimension C, C %% 8 == 0, "
        "8 <= C <= 2048, elementwise_affine: every ConvNeXt, ViT and Swin block) on the native HIP "
        "kernels where the input is a dense GPU tensor under 16-bit autocast; the result then has the "
        "autocast dtype (fp32 LayerNorm, rounded once) instead of fp32; elsewhere (CPU, no autocast, "
        "validation, strided inputs) the modules fall back to F.layer_norm",
        "layernorm", "convert_layernorm", "{0} LayerNorm(s) of {arch} converted"),
    Conversion(
        "bnact",
        "torch engine: run qualifying BatchNorm2d layers (affine, running statistics, channels %% 8 == 0, "
        "<= 2048) fused with the ReLU / ReLU6 / Hardswish that follows them on the native HIP kernels "
        "where the training activations are 16-bit channels_last GPU tensors; elsewhere (CPU, fp32, "
        "validation) the modules fall back to the stock ops; ignored when --sync_batchnorm converts "
        "the model",
        "bnact", "convert_bnact", "{0} BatchNorm(s) of {arch} converted, {1} activation(s) fused",
        syncbn_voids=True),  # and it would drop the absorbed activations
    Conversion(
        "convstats",
        "torch engine, with --native-pointwise on and --native-bnact on: a converted 1x1 conv directly "
        "followed by its converted BatchNorm inside an nn.Sequential forms the BatchNorm statistics in "
        "its own epilogue, so the BatchNorm does not read the conv output again for them; ignored "
        "when either of the two conversions is off or ignored",
        "convstats", "convert_convstats", "{0} conv/BatchNorm pair(s) of {arch} fused",
        needs=("pointwise", "bnact"), syncbn_voids=True),  # pairs of those two conversions
)


# the ops beyond the convolution / normalisation family, run after TABLE in this order
ATTENTION = (
    Conversion(
        "winattn",
        "torch engine: run the window attention of Swin, Swin V2 and MaxViT blocks (head dimension 32, at most 64 "
        "tokens per window, no active attention dropout) on the native HIP kernels where the qkv is a 16-bit GPU "
        "tensor; the relative-position bias stays fp32 and the shift mask is a label table; elsewhere (CPU, fp32, "
        "validation) the modules fall back to F.scaled_dot_product_attention",
        "winattn", "convert_window_attention", "{0} attention module(s) of {arch} converted"),
    Conversion(
        "mha",
        "torch engine: run the global self-attention of ViT blocks (nn.MultiheadAttention, batch first, head "
        "dimension 64, at most 4096 tokens, no mask, no attention weights, no active attention dropout) on the native "
        "HIP kernels where the in-projection comes out as a 16-bit GPU tensor; elsewhere (CPU, fp32, masks, "
        "need_weights) the modules fall back to nn.MultiheadAttention's own forward",
        "mha", "convert_mha", "{0} attention module(s) of {arch} converted"),
    Conversion(
        "se",
        "torch engine: run the squeeze-and-excitation blocks of EfficientNet / V2, MobileNetV3, RegNet-Y and MaxViT "
        "(ReLU or SiLU squeeze, Sigmoid or Hardsigmoid gate, biased 1x1 fc1 / fc2, channels %% 8 == 0 and within "
        "8..4096, squeeze width <= 512) on the native HIP kernels where the input is a 16-bit channels_last GPU "
        "tensor; the gate is then computed in fp32 from the fp32 parameters; elsewhere (CPU, fp32, validation, "
        "wider blocks) the modules fall back to their own forward",
        "se", "convert_se", "{0} squeeze-excitation module(s) of {arch} converted"),
    Conversion(
        "mlp",
        "torch engine: run the channel MLPs of ConvNeXt, Swin and MaxViT blocks (a biased Linear, an exact-erf GELU, "
        "optionally an inactive Dropout and a biased Linear in consecutive slots of an nn.Sequential; widths %% 8 == 0, "
        "in and out within 8..512, hidden within 8..2048) on the native HIP kernels where the input is a dense GPU "
        "tensor under 16-bit autocast: bias, GELU and its derivative are folded into the GEMMs around the hidden "
        "tensor, and the first bias is added in fp32 after that GEMM's 16-bit rounding; wider MLPs (hidden 3072: "
        "ConvNeXt's and Swin's last stage, every ViT block) and everything elsewhere (CPU, fp32, validation, active "
        "dropout) stay on the stock ops",
        "mlp", "convert_mlp", "{0} MLP(s) of {arch} converted"),
)


def add_flags(parser) -> None:
    """One ``--native-<name> {off,on}`` flag (default off) per record on ``parser`` (or an argument group)."""
    for c in TABLE + ATTENTION:
        parser.add_argument("--native-" + c.name, default="off", choices=["off", "on"], help=c.help)


def apply(model, flags, arch: str, syncbn_converts: bool, say) -> dict:
    """Run on ``model``, in table order (``TABLE``, then ``ATTENTION``), every conversion whose ``flags.native_<name>``
    is ``"on"`` (a missing attribute is off) and report each through ``say(line)``: what it converted, or why it is
    ignored (a missing prerequisite first, then ``syncbn_converts``: the caller will turn the BatchNorms into SyncBatchNorm).  Returns
    ``{name: tuple of counts}`` of the conversions that ran.  Call it before the parameters are flattened: the converted
    modules keep the same ``Parameter`` objects."""
    def on(name):
        return getattr(flags, "native_" + name, "off") == "on"

    counts = {}
    for c in TABLE + ATTENTION:
        if not on(c.name):
            continue
        if not all(on(n) for n in c.needs):
            line = "ignored, it needs " + " and ".join("--native-{} on".format(n) for n in c.needs)
        elif c.syncbn_voids and syncbn_converts:
            line = "ignored, --sync_batchnorm converts the model's BatchNorms"
        else:
            got = getattr(importlib.import_module("." + c.module, __package__), c.function)(model)
            counts[c.name] = got if isinstance(got, tuple) else (got,)
            line = c.result.format(*counts[c.name], arch=arch)
        say("=> native {}: {}".format(c.name, line))
    return counts
