"""Static architecture tables for the three networks on the hot path.

These tables are the single source of truth for (a) the state_dict key contract the drop-in
modules must honour, (b) the flat parameter-buffer layout that the C-ABI
library consumes (include/dvc_hip.h, "parameter packing"), and (c) the synthetic weight
factory in ``synth.py``.

Shapes follow the reference constructors:
  VGG19_pytorch   /root/reference/models/NonlocalNet.py:197-226
  WarpNet         /root/reference/models/NonlocalNet.py:358-425
  ColorVidNet     /root/reference/models/ColorVidNet.py:7-94

Next to each table stands what the layer walks of ``nets.py`` need to know about its structure (VGG_POOL_AFTER,
WARP_HEAD_PLAN, CVN_GRAPH): derived once, here, immutable, and free of torch, so the relations can be read and tested
without a device.
"""
from collections import namedtuple
from types import MappingProxyType
from typing import NamedTuple

# ---------------------------------------------------------------------------------------------
# VGG19: 16 conv3x3 (pad 1) + ReLU, 5 maxpool2x2.  (name, cin, cout)
VGG_CONVS = [
    ("conv1_1", 3, 64), ("conv1_2", 64, 64),
    ("conv2_1", 64, 128), ("conv2_2", 128, 128),
    ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv3_4", 256, 256),
    ("conv4_1", 256, 512), ("conv4_2", 512, 512), ("conv4_3", 512, 512), ("conv4_4", 512, 512),
    ("conv5_1", 512, 512), ("conv5_2", 512, 512), ("conv5_3", 512, 512), ("conv5_4", 512, 512),
]
# forward order of activation keys (NonlocalNet.py:235-256); "p*" are the pools
VGG_KEYS = [
    "r11", "r12", "p1", "r21", "r22", "p2", "r31", "r32", "r33", "r34", "p3",
    "r41", "r42", "r43", "r44", "p4", "r51", "r52", "r53", "r54", "p5",
]
VGG_CONV_OF = MappingProxyType({"r" + n[4:].replace("_", ""): n for n, _, _ in VGG_CONVS})    # output key "r12" -> "conv1_2"
VGG_POOL_AFTER = frozenset(k for k, nxt in zip(VGG_KEYS, VGG_KEYS[1:]) if k[0] == "r" and nxt[0] == "p")

# ---------------------------------------------------------------------------------------------
# WarpNet feature heads: list of (state_dict conv index, cin, cout, stride, prelu index).
# layer5_1 has an extra Upsample between its two convs so its indices differ
# (NonlocalNet.py:364-410).
WARP_HEADS = {
    "layer2_1": dict(convs=[(1, 128, 128, 1, 3), (5, 128, 64, 2, 7)], up_mid=False, up_out=False),
    "layer3_1": dict(convs=[(1, 256, 128, 1, 3), (5, 128, 64, 1, 7)], up_mid=False, up_out=False),
    "layer4_1": dict(convs=[(1, 512, 256, 1, 3), (5, 256, 64, 1, 7)], up_mid=False, up_out=True),
    "layer5_1": dict(convs=[(1, 512, 256, 1, 3), (6, 256, 64, 1, 8)], up_mid=True, up_out=True),
}
WARP_HEAD_ORDER = ["layer2_1", "layer3_1", "layer4_1", "layer5_1"]
WARP_FEATURE_CH = 64
WARP_TRUNK_CH = 256          # 4 heads x 64 channels, also theta/phi inter_channels
WARP_NUM_RESBLOCKS = 3


# One head as WarpNet._heads walks it: conv_a -> norm + PReLU prelu_a -> [x2 up_mid] -> conv_b (stride_b) -> norm + PReLU prelu_b
# -> [x2 up_out]; conv_* / prelu_* are positions in the head's Sequential.  (The first convolution's stride is 1 in every head.)
WarpHead = namedtuple("WarpHead", "index name conv_a prelu_a conv_b stride_b prelu_b up_mid up_out")


def _warp_head(index, name):
    (ia, _, _, _, pa), (ib, _, _, sb, pb) = WARP_HEADS[name]["convs"]
    return WarpHead(index, name, ia, pa, ib, sb, pb, WARP_HEADS[name]["up_mid"], WARP_HEADS[name]["up_out"])


WARP_HEAD_PLAN = tuple(_warp_head(i, name) for i, name in enumerate(WARP_HEAD_ORDER))


def warp_head_out_hw(name, H, W):
    """Output size of the head `name` on an H x W feature map (the 3x3 convolutions reflect-pad by 1: only the stride and the
    two upsamples move the size)."""
    hd = WARP_HEAD_PLAN[WARP_HEAD_ORDER.index(name)]
    if hd.up_mid:
        H, W = 2 * H, 2 * W
    H, W = (H - 1) // hd.stride_b + 1, (W - 1) // hd.stride_b + 1
    if hd.up_out:
        H, W = 2 * H, 2 * W
    return H, W


def warp_trunk_geometry(shapes_in):
    """(h, w, rpad5) of the trunk tensor from the (H, W) of the four heads' inputs, in WARP_HEAD_ORDER.  rpad5 = 1: layer5_1's
    output is short of layer2_1's and gets one replicated row top and bottom (NonlocalNet.py:461-463)."""
    shapes = [warp_head_out_hw(name, H, W) for name, (H, W) in zip(WARP_HEAD_ORDER, shapes_in)]
    h, w = shapes[0]
    rpad5 = 0
    if shapes[3] != shapes[0]:
        rpad5 = 1
        shapes[3] = (shapes[3][0] + 2, shapes[3][1])
    for nm, sh in zip(WARP_HEAD_ORDER, shapes):
        if sh != (h, w):
            raise RuntimeError(f"Sizes of tensors must match except in dimension 1: {nm} gives {sh}, "
                               f"layer2_1 gives {(h, w)}")
    return h, w, rpad5


def warpnet_param_shapes():
    """Ordered {key: shape} for WarpNet.state_dict() (43 tensors)."""
    out = {}
    for name in WARP_HEAD_ORDER:
        for (ci, cin, cout, _s, pi) in WARP_HEADS[name]["convs"]:
            out[f"{name}.{ci}.weight"] = (cout, cin, 3, 3)
            out[f"{name}.{ci}.bias"] = (cout,)
            out[f"{name}.{pi}.weight"] = (1,)
    for b in range(WARP_NUM_RESBLOCKS):
        for cv in ("conv1", "conv2"):
            out[f"layer.{b}.{cv}.weight"] = (WARP_TRUNK_CH, WARP_TRUNK_CH, 3, 3)
            out[f"layer.{b}.{cv}.bias"] = (WARP_TRUNK_CH,)
        out[f"layer.{b}.prelu.weight"] = (1,)
    for nm in ("theta", "phi"):
        out[f"{nm}.weight"] = (WARP_TRUNK_CH, WARP_TRUNK_CH, 1, 1)
        out[f"{nm}.bias"] = (WARP_TRUNK_CH,)
    return out


def vgg_param_shapes():
    out = {}
    for (name, cin, cout) in VGG_CONVS:
        out[f"{name}.weight"] = (cout, cin, 3, 3)
        out[f"{name}.bias"] = (cout,)
    return out


# ---------------------------------------------------------------------------------------------
# ColorVidNet: conv list in *execution* order.  Each entry:
#   key      state_dict prefix (".weight"/".bias" appended)
#   cin,cout
#   dil      dilation (pad == dil for all 3x3 convs here)
#   src      name of the activation this conv reads
#   pre      how the source is transformed on load:
#              None      as stored
#              "norm"    InstanceNorm of src (eps 1e-5, biased var)
#              "norm_ss" InstanceNorm -> depthwise 1x1 stride-2 scale (`*_ss.weight`)
#              "up"      InstanceNorm -> nearest x2 upsample
#   add      name of an activation added to the conv output before the activation (or None)
#   act      "relu" | "none" | "leaky" | "tanh128"
#   dst      name the result is stored under
# (ColorVidNet.py:96-144)
CVN_CONVS = [
    dict(key="conv1_1.0", cin=None, cout=32, dil=1, src="x", pre=None, add=None, act="relu", dst="c1_1a"),
    dict(key="conv1_1.2", cin=32, cout=64, dil=1, src="c1_1a", pre=None, add=None, act="relu", dst="c1_1"),
    dict(key="conv1_2", cin=64, cout=64, dil=1, src="c1_1", pre=None, add=None, act="relu", dst="c1_2"),
    dict(key="conv2_1", cin=64, cout=128, dil=1, src="c1_2", pre="norm_ss", ss="conv1_2norm_ss", add=None, act="relu", dst="c2_1"),
    dict(key="conv2_2", cin=128, cout=128, dil=1, src="c2_1", pre=None, add=None, act="relu", dst="c2_2"),
    dict(key="conv3_1", cin=128, cout=256, dil=1, src="c2_2", pre="norm_ss", ss="conv2_2norm_ss", add=None, act="relu", dst="c3_1"),
    dict(key="conv3_2", cin=256, cout=256, dil=1, src="c3_1", pre=None, add=None, act="relu", dst="c3_2"),
    dict(key="conv3_3", cin=256, cout=256, dil=1, src="c3_2", pre=None, add=None, act="relu", dst="c3_3"),
    dict(key="conv4_1", cin=256, cout=512, dil=1, src="c3_3", pre="norm_ss", ss="conv3_3norm_ss", add=None, act="relu", dst="c4_1"),
    dict(key="conv4_2", cin=512, cout=512, dil=1, src="c4_1", pre=None, add=None, act="relu", dst="c4_2"),
    dict(key="conv4_3", cin=512, cout=512, dil=1, src="c4_2", pre=None, add=None, act="relu", dst="c4_3"),
    dict(key="conv5_1", cin=512, cout=512, dil=2, src="c4_3", pre="norm", add=None, act="relu", dst="c5_1"),
    dict(key="conv5_2", cin=512, cout=512, dil=2, src="c5_1", pre=None, add=None, act="relu", dst="c5_2"),
    dict(key="conv5_3", cin=512, cout=512, dil=2, src="c5_2", pre=None, add=None, act="relu", dst="c5_3"),
    dict(key="conv6_1", cin=512, cout=512, dil=2, src="c5_3", pre="norm", add=None, act="relu", dst="c6_1"),
    dict(key="conv6_2", cin=512, cout=512, dil=2, src="c6_1", pre=None, add=None, act="relu", dst="c6_2"),
    dict(key="conv6_3", cin=512, cout=512, dil=2, src="c6_2", pre=None, add=None, act="relu", dst="c6_3"),
    dict(key="conv7_1", cin=512, cout=512, dil=1, src="c6_3", pre="norm", add=None, act="relu", dst="c7_1"),
    dict(key="conv7_2", cin=512, cout=512, dil=1, src="c7_1", pre=None, add=None, act="relu", dst="c7_2"),
    dict(key="conv7_3", cin=512, cout=512, dil=1, src="c7_2", pre=None, add=None, act="relu", dst="c7_3"),
    dict(key="conv3_3_short", cin=256, cout=256, dil=1, src="c3_3", pre="norm", add=None, act="none", dst="s3"),
    dict(key="conv8_1.1", cin=512, cout=256, dil=1, src="c7_3", pre="up", add="s3", act="relu", dst="c8_1"),
    dict(key="conv8_2", cin=256, cout=256, dil=1, src="c8_1", pre=None, add=None, act="relu", dst="c8_2"),
    dict(key="conv8_3", cin=256, cout=256, dil=1, src="c8_2", pre=None, add=None, act="relu", dst="c8_3"),
    dict(key="conv2_2_short", cin=128, cout=128, dil=1, src="c2_2", pre="norm", add=None, act="none", dst="s2"),
    dict(key="conv9_1.1", cin=256, cout=128, dil=1, src="c8_3", pre="up", add="s2", act="relu", dst="c9_1"),
    dict(key="conv9_2", cin=128, cout=128, dil=1, src="c9_1", pre=None, add=None, act="relu", dst="c9_2"),
    dict(key="conv1_2_short", cin=64, cout=128, dil=1, src="c1_2", pre="norm", add=None, act="none", dst="s1"),
    dict(key="conv10_1.1", cin=128, cout=128, dil=1, src="c9_2", pre="up", add="s1", act="relu", dst="c10_1"),
    dict(key="conv10_2", cin=128, cout=128, dil=1, src="c10_1", pre=None, add=None, act="leaky", dst="c10_2"),
]
CVN_SS = [("conv1_2norm_ss", 64), ("conv2_2norm_ss", 128), ("conv3_3norm_ss", 256)]
CVN_OUT = dict(key="conv10_ab", cin=128, cout=2, src="c10_2")   # 1x1 conv then tanh*128 (ColorVidNet.py:142-144)


class CvnGraph(NamedTuple):
    """Who reads what in CVN_CONVS + CVN_OUT, for ColorVidNet's forward and backward walks.  "Activation" = a `dst` name."""
    by_key: MappingProxyType            # conv key -> its entry (read-only view)
    by_dst: MappingProxyType            # activation -> the entry that produces it
    norm_variants: MappingProxyType     # activation -> the InstanceNorm forms to materialise right after it is produced, in
                                        # consumer order without repeats: None = plain, or the `_ss` key (scaled, stride 2)
    norm_pair: MappingProxyType         # activation -> `_ss` key where both forms are wanted: one launch produces the two
    ss_of: MappingProxyType             # activation -> the `_ss` key that scales its norm
    norm_only: frozenset                # activations read only through a norm: the producer may leave its split-K reduce to it
    dual: MappingProxyType              # consumer key -> the key of the skip convolution it adds, where the two can run as ONE
                                        # launch: a linear convolution read by nothing else, same dilation
    skip_keys: frozenset                # those skip convolutions: they run with their consumer, not at their place in the table
    adder: MappingProxyType             # skip output -> the activation of the block it is added into
    grad_kind: MappingProxyType         # `pre` -> the slot of cvn_inorm_bwd a consumer's input gradient goes to ("raw": no norm)
    saved_acts: tuple                   # activations behind a nonlinearity: what the backward needs saved


def _cvn_graph(convs, out):
    by_key = {c["key"]: MappingProxyType(c) for c in convs}
    by_dst = {c["dst"]: by_key[c["key"]] for c in convs}
    norm_uses, raw_use, uses = {}, {out["src"]}, {}
    for c in convs:
        if c["pre"] is None:
            raw_use.add(c["src"])
        else:
            norm_uses.setdefault(c["src"], []).append(c["ss"] if c["pre"] == "norm_ss" else None)
        if c["add"] is not None:
            raw_use.add(c["add"])
        for a in (c["src"], c["add"]):
            uses[a] = uses.get(a, 0) + 1
    norm_variants = {a: tuple(dict.fromkeys(v)) for a, v in norm_uses.items()}
    ss_of = {c["src"]: c["ss"] for c in convs if c["pre"] == "norm_ss"}
    dual = {}
    for c in convs:
        e = by_dst.get(c["add"])
        if e is not None and e["act"] == "none" and e["add"] is None and uses[e["dst"]] == 1 and e["dil"] == c["dil"] \
                and e["pre"] in (None, "norm") and c["pre"] in ("up", "norm", None):
            dual[c["key"]] = e["key"]
    ro = MappingProxyType
    return CvnGraph(
        by_key=ro(by_key), by_dst=ro(by_dst), norm_variants=ro(norm_variants),
        norm_pair=ro({a: k for a, k in ss_of.items() if None in norm_variants[a]}), ss_of=ro(ss_of),
        norm_only=frozenset(norm_uses) - raw_use, dual=ro(dual), skip_keys=frozenset(dual.values()),
        adder=ro({c["add"]: c["dst"] for c in convs if c["add"] is not None}),
        grad_kind=ro({None: "raw", "norm": "full", "norm_ss": "ss", "up": "up"}),
        saved_acts=tuple(c["dst"] for c in convs if c["act"] != "none"))


CVN_GRAPH = _cvn_graph(CVN_CONVS, CVN_OUT)

# state_dict key order of the reference module (registration order in ColorVidNet.__init__,
# with conv8_1/9_1/10_1 re-registered in place as Sequential(Upsample, Conv2d)).
CVN_STATE_ORDER = [
    ("conv1_1.0", "conv"), ("conv1_1.2", "conv"), ("conv1_2", "conv"), ("conv1_2norm_ss", "ss"),
    ("conv2_1", "conv"), ("conv2_2", "conv"), ("conv2_2norm_ss", "ss"),
    ("conv3_1", "conv"), ("conv3_2", "conv"), ("conv3_3", "conv"), ("conv3_3norm_ss", "ss"),
    ("conv4_1", "conv"), ("conv4_2", "conv"), ("conv4_3", "conv"),
    ("conv5_1", "conv"), ("conv5_2", "conv"), ("conv5_3", "conv"),
    ("conv6_1", "conv"), ("conv6_2", "conv"), ("conv6_3", "conv"),
    ("conv7_1", "conv"), ("conv7_2", "conv"), ("conv7_3", "conv"),
    ("conv8_1.1", "conv"), ("conv3_3_short", "conv"), ("conv8_2", "conv"), ("conv8_3", "conv"),
    ("conv9_1.1", "conv"), ("conv2_2_short", "conv"), ("conv9_2", "conv"),
    ("conv10_1.1", "conv"), ("conv1_2_short", "conv"), ("conv10_2", "conv"), ("conv10_ab", "conv"),
]


def colorvidnet_param_shapes(ic=7):
    by_key = {c["key"]: c for c in CVN_CONVS}
    ss = dict(CVN_SS)
    out = {}
    for key, kind in CVN_STATE_ORDER:
        if kind == "ss":
            out[f"{key}.weight"] = (ss[key], 1, 1, 1)
            continue
        if key == CVN_OUT["key"]:
            out[f"{key}.weight"] = (CVN_OUT["cout"], CVN_OUT["cin"], 1, 1)
            out[f"{key}.bias"] = (CVN_OUT["cout"],)
            continue
        c = by_key[key]
        cin = ic if c["cin"] is None else c["cin"]
        out[f"{key}.weight"] = (c["cout"], cin, 3, 3)
        out[f"{key}.bias"] = (c["cout"],)
    return out


# ---------------------------------------------------------------------------------------------
# Error-aware engine map (ops.direct_layers): the 3x3 layers that stay on the direct implicit-GEMM engine under the default
# algorithm choice because their Winograd rounding moves the frame's ab output the most per microsecond saved
# (tools/engine_sensitivity.py on the MI355X, profiles/r05_engine_sensitivity.txt).  Names = state_dict prefixes with the
# network in front ("vgg.", "warp.", "cvn.").
# What the measurements say (r05, MI355X, 216x384, plain seed-0 weights, T = 1e-10, 10 frames without arg-max flips against the
# fp64 oracle, CPU fp32 = 1.00; profiles/r05_engine_map_eval.txt):
#   every eligible layer on Winograd ("speed")        rms 1.10  mean 1.09  q999 1.16  max 1.92
#   the whole FRONT END direct, ColorVidNet Winograd  rms 1.09  — the front end's engine does not matter: at T = 1e-10 it reaches
#                                                       ColorVidNet only through the similarity map's last bits and the arg-max
#   ColorVidNet direct, front end Winograd            rms 0.81  — the same as everything direct (0.82)
#   conv2_1, conv2_2 direct                           rms 0.99  mean 0.98  q999 1.02  max 1.72
#   conv1_1.2 .. conv2_2 direct                       rms 0.91  mean 0.91  q999 0.94  max 1.26
#   conv1_1.2 .. conv3_3 direct (this map)            rms 0.85  mean 0.85  q999 0.85  max 0.91   (worst frame: max 1.06)
# The excess sits in ColorVidNet's first seven 3x3 layers (an error there is amplified by everything behind it: perturbation
# energy per layer falls 30x from conv1_2 to conv4_3, profiles/r05_engine_sensitivity.txt, while Winograd's own rounding is
# 1.1-2.2x the direct sum's on every layer, profiles/r05_engine_layer_error.txt); they cost 107-135 us of convolution time per
# frame on the direct engine.  Forcing a larger split over input channels on the Winograd kernel (shorter accumulation chains)
# buys less accuracy per microsecond than the direct engine on every one of them (same file).
# r06: re-evaluated with tools/parity_pool_probe.py (8 frames without arg-max flips, profiles/r06_parity_pool_probe_maps.txt) now
# that five of the seven layers run on the weights-in-registers kernel: without conv3_3 (the 256 -> 256 layer at 54x96 right in
# front of an InstanceNorm: as a Winograd launch it also leaves its split-K reduce to that norm's launch) the pooled statistics
# are max 1.01, q99.9 0.90, mean 0.87, rms 0.88 of the CPU fp32 run's — the seven-layer map: 1.03 / 0.90 / 0.86 / 0.86 — for 25 us
# per frame less; without conv3_2 as well q99.9 reaches 1.01 (mean 0.90), so that one stays.
DIRECT_LAYERS = frozenset(("cvn.conv1_1.2", "cvn.conv1_2", "cvn.conv2_1", "cvn.conv2_2", "cvn.conv3_1", "cvn.conv3_2"))


# ---------------------------------------------------------------------------------------------
# Discriminator_x64 (models/GAN_models.py:104-157): six spectrally normalised 4x4 stride-2 pad-1 convolutions + LeakyReLU(0.2),
# the self-attention block between layer4 and layer5, then the [3, 6] valid convolution `last` and the mean over its positions.
GAN_LAYERS = ("layer1", "layer2", "layer3", "layer4", "layer5", "layer6")
GAN_CH_MULT = (1, 1, 2, 4, 8, 16)            # Cout / ndf of layer1 .. layer6
GAN_ATTENTION_AFTER = "layer4"
GAN_ATTENTION_CONVS = ("query_conv", "key_conv", "value_conv")
GAN_LAST_KSIZE = (3, 6)
GAN_LRELU_SLOPE = 0.2
GAN_SN_EPS = 1e-12


def gan_conv_plan(in_size=6, ndf=64):
    """[(name, cin, cout)] of layer1 .. layer6."""
    chans = [in_size] + [m * ndf for m in GAN_CH_MULT]
    return [(name, chans[i], chans[i + 1]) for i, name in enumerate(GAN_LAYERS)]


def gan_out_hw(H, W):
    """The map `last` sees: six halvings, each rounding down."""
    for _ in GAN_LAYERS:
        H, W = H // 2, W // 2
    return H, W


def discriminator_param_shapes(in_size=6, ndf=64):
    """state_dict key -> shape, in the reference's order: per SpectralNorm module bias, weight_u, weight_v, weight_bar."""
    def sn(prefix, cout, cin, kh, kw):
        return {prefix + ".bias": (cout,), prefix + ".weight_u": (cout,), prefix + ".weight_v": (cin * kh * kw,),
                prefix + ".weight_bar": (cout, cin, kh, kw)}
    shapes = {}
    plan = gan_conv_plan(in_size, ndf)
    for name, cin, cout in plan:
        shapes.update(sn(name + ".0.module", cout, cin, 4, 4))
        if name == GAN_ATTENTION_AFTER:
            shapes["attention.gamma"] = (1,)
            for conv in GAN_ATTENTION_CONVS:
                shapes.update(sn(f"attention.{conv}.module", cout, cout, 1, 1))
    shapes.update(sn("last.module", 1, plan[-1][2], *GAN_LAST_KSIZE))
    return shapes
