"""Drop-in nn.Module classes for the hot path, backed by the HIP kernels.

Same constructor arguments, forward signatures, return conventions and state_dict keys as
  VGG19_pytorch  /root/reference/models/NonlocalNet.py:192-256
  WarpNet        /root/reference/models/NonlocalNet.py:355-502
  ColorVidNet    /root/reference/models/ColorVidNet.py:6-144
so `load_state_dict(torch.load(...))`, `.parameters()`, `.eval()`, `.cuda()` behave as in
/root/reference/test.py:147-166.  The torch.nn submodules created here are *parameter containers
only* (they give the parameters their reference names); no torch.nn forward is ever called — every
forward pass is a sequence of libdvc_hip.so kernel launches on the current stream.

Inference only, with two exceptions: VGG19_pytorch gives the input gradient (frozen weights) that the reference's training
losses need (train.py:649-668 take the perceptual and contextual losses on the features of the predicted frame), and
ColorVidNet in training mode (`colornet.train()`, grad mode on, the input or a parameter requiring grad) gives the gradients
of all its parameters and of its input (train.py trains it).  WarpNet in training mode (`nonlocal_net.train()`, grad mode on, a
parameter of layer.* / theta / phi requiring grad, the four heads frozen) gives the gradients of its residual trunk and of the
theta / phi projections; its heads and its inputs carry no history.  `nonlocal_net.set_head_training()` opts in to the heads'
24 gradients as well: the four heads need not be frozen then, and only the inputs stay data.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import arch, ops

_VGG_MEAN_BGR = (0.40760392, 0.45795686, 0.48501961)  # utils/util.py:351


_pack_epoch = 0


def pack_epoch():
    """Number of weight (re)packs so far in this process: a captured launch sequence (dvc_amd/graph.py) bakes the packed
    tensors' addresses in and is re-captured when this has moved (load_state_dict, .cuda(), another conv algorithm)."""
    return _pack_epoch


class _PackCache:
    """Repacked weights ([Cin][k*k][Cout]) keyed by parameter identity + version, so an in-place
    `load_state_dict` or a `.cuda()` move is picked up on the next forward."""

    def __init__(self):
        self._d = {}

    def get(self, key, param, fn):
        """`param`: a parameter, or a tuple of parameters (fn then receives the tuple) — e.g. the concatenated filters of two
        convolutions that run as one launch."""
        params = param if isinstance(param, tuple) else (param,)
        tag = tuple((p.data_ptr(), _version_of(p), str(p.device)) for p in params)
        param = params[0]
        hit = self._d.get(key)
        if hit is None or hit[0] != tag:
            # Cold path (first use, or after load_state_dict / .cuda()).  The packed tensor is produced
            # on whatever stream is current and then read by kernels on ANY stream (the clip driver runs
            # front ends on side streams), so the miss is made a device-wide ordering point: everything
            # that may still read the entry being replaced has finished before it is dropped, and the new
            # entry is complete before any stream can see it.  `prepare()` takes all misses up front.
            if param.is_cuda:
                torch.cuda.synchronize(param.device)
            global _pack_epoch
            _pack_epoch += 1
            with torch.no_grad():
                hit = (tag, fn(params if len(params) > 1 else param))
            if param.is_cuda:
                torch.cuda.synchronize(param.device)
            self._d[key] = hit
        return hit[1]


def invalidate_weight_caches(*modules):
    """Forget every packed filter (and the exemplar memo) of the given modules: the next forward repacks from the current
    parameter values.  Needed only after writing parameters THROUGH `.data` (`p.data.copy_(...)`), which moves no version
    counter; `load_state_dict`, `.cuda()` and in-place operations on the Parameter itself are noticed without it.  Captured
    launch sequences re-capture (pack_epoch moves); a ClipColorizer's cached exemplar side does not know: call its
    `set_exemplar` again when VGG19 / WarpNet weights were rewritten this way."""
    global _pack_epoch
    for m in modules:
        cache = getattr(m, "_cache", None)
        if isinstance(cache, _PackCache):
            if any(p.is_cuda for p in m.parameters()):
                torch.cuda.synchronize()
            cache._d.clear()
        if getattr(m, "_exemplar_memo", None) is not None:
            object.__setattr__(m, "_exemplar_memo", None)
    _pack_epoch += 1


def _version_of(t):
    """`t._version`, or None for a tensor without a version counter (created under torch.inference_mode())."""
    try:
        return t._version
    except RuntimeError:
        return None


def _same_tensors(a, b):
    """Bit-for-bit equality of two nested tuples of tensors (non-tensor leaves compare with ==)."""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same_tensors(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))
    return a == b


def _packs(cache, key, weight, transform=None):
    """kind -> packed weight of one 3x3 layer: "direct" = [Cin][9][Cout], "winograd" = U = G g G^T (ops.conv3x3).
    transform: applied to the weight before it is packed (a backward walk's input-gradient filters)."""
    def get(kind):
        if kind == "winograd":
            suffix, pack = ":wino", ops.pack_winograd_weight
        elif kind == "ws":
            suffix, pack = ":ws", ops.pack_ws_weight
        else:
            suffix, pack = "", ops.pack_conv_weight
        return cache.get(key + suffix, weight, pack if transform is None else lambda w: pack(transform(w)))
    return get


def _bwd_filters(cache, key, weight, transform):
    """What ops.conv3x3 takes for a 3x3 layer's input gradient: (the transformed filters themselves, cached under key + ":wt",
    and their `_packs` under key / key + ":wino" / key + ":ws").  key: "<net>_bwd.<layer>"; transform: vgg_bwd_weight or
    cvn_bwd_weight (W^T flipped)."""
    return cache.get(key + ":wt", weight, transform), _packs(cache, key, weight, transform)


def _save_dict(ctx, tensors):
    """Put a dict of tensors on an autograd ctx (save_for_backward); _saved_dict(ctx) gives it back in backward."""
    ctx.saved_keys = tuple(tensors)
    ctx.save_for_backward(*tensors.values())


def _saved_dict(ctx):
    return dict(zip(ctx.saved_keys, ctx.saved_tensors))


def _wants(need, prefix):
    """Is the weight or the bias gradient of the layer `prefix` asked for?"""
    return prefix + ".weight" in need or prefix + ".bias" in need


def _put_wb(grads, need, prefix, dW, db):
    """Store dW / db under prefix.weight / prefix.bias, each only if its name is in `need`."""
    for name, g in ((prefix + ".weight", dW), (prefix + ".bias", db)):
        if name in need:
            grads[name] = g


def _check_trainable(named, who):
    """The training paths launch on the parameters' storage: those that take a gradient are float32 ROCm tensors."""
    for n, p in named:
        if p.requires_grad and (not p.is_cuda or p.dtype != torch.float32):
            raise RuntimeError(f"{who}: parameter {n} must be a float32 ROCm tensor for the training path")


def _prepack(cache, key, conv):
    """Both packed forms a 3x3 layer may be asked for under the current algorithm choice (ops.set_conv_algo)."""
    get = _packs(cache, key, conv.weight)
    get("direct")
    co, ci, kh, kw = conv.weight.shape
    if ops.conv_algo() != "direct" and conv.stride[0] == 1 and ops.winograd_eligible(ci, co, kh):
        get("winograd")
    if ops.ws_conv_enabled() and conv.stride[0] == 1 and kh == 3 and ops.ws_eligible(ci, co):
        get("ws")


def _norm_in_place(t, **kw):
    """InstanceNorm (+ what follows) of a convolution output, in place — or, when the convolution left its split-K partial
    sums for this launch to add up (ops.ConvPartials), into a new tensor."""
    return ops.instnorm_apply(t, out=None if isinstance(t, ops.ConvPartials) else t, **kw)


def _check_input(x, name):
    if not x.is_cuda:
        raise RuntimeError(f"{name}: input is on {x.device}; the MI355X HIP path has no CPU fallback "
                           "(move the module and its inputs to the GPU with .cuda())")
    if x.requires_grad and torch.is_grad_enabled():
        # the reference would record an autograd graph here (train.py:402-427); this forward is
        # inference-only, so say so instead of silently returning a tensor without history
        raise NotImplementedError(
            f"{name}: an input requires grad and autograd is enabled, but this forward is inference-only. Call it under "
            "torch.no_grad() as test.py:83 does, or detach the input; gradients exist for ColorVidNet in training mode "
            "(`colornet.train()`: parameters and input), WarpNet in training mode (`nonlocal_net.train()`: the residual trunk "
            "and the theta / phi projections, heads frozen — or all 43 parameters after `nonlocal_net.set_head_training()`; its "
            "inputs are data), VGG19_pytorch.forward (input gradient, frozen "
            "weights), tensor_lab2rgb, the fused correlation (dvc_amd.corr_autograd) and the contextual losses.")


def vgg_bwd_weight(w):
    """The filters of a 3x3 stride-1 pad-1 convolution's input gradient: dL/dx = conv3x3(dL/dy, W^T flipped), [Cin][Cout][3][3]
    — Cin and Cout swap places at the same H x W, so the forward's engines (ops.conv3x3) run it as they are."""
    return w.detach().transpose(0, 1).flip(2, 3).contiguous()


def vgg_bwd_weight_conv1(w, preprocess=True):
    """conv1_1's [3][Cout][3][3] input-gradient filters (ops.vgg_conv1_bwd).  preprocess=True folds vgg_preprocess
    (utils/util.py:347-352: x_bgr[c] = (x_rgb[2 - c] - mean[c]) * 255) in, so the result is d/d rgb: the output channels in
    reverse order, times 255."""
    wt = vgg_bwd_weight(w)
    return (wt.flip(0) * 255.0).contiguous() if preprocess else wt


class _VGGInputGrad(torch.autograd.Function):
    """VGG19_pytorch.forward with the post-ReLU output of every convolution up to the deepest requested key saved; backward walks
    the layers in reverse and returns d x only (the weights are frozen)."""

    @staticmethod
    def forward(ctx, x, module, out_keys, preprocess):
        saved = {}
        outs = module._forward(x, out_keys, preprocess, False, saved=saved)
        ctx.module, ctx.out_keys, ctx.preprocess = module, tuple(out_keys), preprocess
        _save_dict(ctx, saved)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        saved = _saved_dict(ctx)
        g_ext = {k: g.contiguous() for k, g in zip(ctx.out_keys, grads) if g is not None}
        return ctx.module._input_grad(saved, g_ext, ctx.preprocess), None, None, None


# ================================================================================================ VGG19
def _check_vgg_keys(out_keys):
    for k in out_keys:
        if k not in arch.VGG_KEYS:
            raise KeyError(k)


class VGG19_pytorch(nn.Module):
    """NOTE: input tensor should range in [0,1] (RGB); see NonlocalNet.py:193-195."""

    def __init__(self, pool="max"):
        super().__init__()
        for name, cin, cout in arch.VGG_CONVS:
            setattr(self, name, nn.Conv2d(cin, cout, kernel_size=3, padding=1))
        if pool not in ("max", "avg"):
            raise ValueError("pool must be 'max' or 'avg'")
        self._pool = pool
        self._cache = _PackCache()

    def _packed(self, name, swap_bgr=False):
        conv = getattr(self, name)
        if swap_bgr:  # fold RGB->BGR of vgg_preprocess into conv1_1's input-channel order
            return self._cache.get(name + ":bgr", conv.weight, lambda w: ops.pack_conv_weight(w.flip(1)))
        return self._cache.get(name, conv.weight, ops.pack_conv_weight)

    def _pre_affine(self, N=1):
        """vgg_preprocess (utils/util.py:347-352) as a per-(image, channel) affine on the stored R,G,B channels:
        BGR channel c' = 2-c gets (x - mean[c'])*255 = x*255 - 255*mean[c'].  [N*3] each, built once per batch size."""
        w = self.conv1_1.weight
        sc = self._cache.get(f"pre:scale:{N}", w, lambda w: torch.full((3 * N,), 255.0, device=w.device))
        sh = self._cache.get(f"pre:shift:{N}", w, lambda w: torch.tensor(
            [-255.0 * _VGG_MEAN_BGR[2], -255.0 * _VGG_MEAN_BGR[1], -255.0 * _VGG_MEAN_BGR[0]] * N, device=w.device))
        return sc, sh

    def prepare(self):
        """Pack every weight now, on the current stream (see _PackCache.get)."""
        for name, _, _ in arch.VGG_CONVS:
            _prepack(self._cache, name, getattr(self, name))
        self._packed("conv1_1", swap_bgr=True)
        self._pre_affine()

    def forward_gray(self, IA_l, out_keys):
        """forward(gray2rgb_batch(IA_l), out_keys, preprocess=True) — the call FrameColor.py:8-10 makes — with the grey-to-RGB
        replication folded into conv1_1's load (DVC_CONV_GRAY_INPUT): IA_l is the centred luminance [N,1,H,W] (a channel slice
        of the Lab frame is fine).  Bit-identical to the two-step form, one launch and a 1 MB tensor less per frame."""
        return self.forward(IA_l, out_keys, preprocess=True, _gray=True)

    def forward(self, x, out_keys, preprocess=True, _gray=False):
        if not _gray and x.is_cuda and x.requires_grad and torch.is_grad_enabled():
            return self._forward_with_grad(x, out_keys, preprocess)
        _check_input(x, "VGG19_pytorch")
        return self._forward(x, out_keys, preprocess, _gray)

    def _forward_with_grad(self, x, out_keys, preprocess):
        """The training path (train.py:649-668): outputs bit-identical to the no-grad forward, with a backward to x."""
        if any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(
                "VGG19_pytorch: only the input gradient is built (no weight gradients); freeze the parameters as train.py "
                "does (`for p in vggnet.parameters(): p.requires_grad = False`)")
        _check_vgg_keys(out_keys)
        if not out_keys:
            return []
        uniq = list(dict.fromkeys(out_keys))    # (a key requested twice: the same tensor twice, autograd adds its gradients)
        outs = _VGGInputGrad.apply(x, self, uniq, preprocess)
        return [outs[uniq.index(k)] for k in out_keys]

    def _input_grad(self, saved, g_ext, preprocess):
        """d x from the saved post-ReLU outputs R and the incoming gradients of the requested keys.  Layer by layer, deepest
        first: dZ = (dX + g(r)) * [R > 0] (ops.vgg_act_bwd), or through a pool (ops.vgg_pool_act_bwd), then the convolution's
        input gradient dX = conv3x3(dZ, W^T flipped) on the forward's engines; conv1_1's 3-channel one on ops.vgg_conv1_bwd."""
        keys = arch.VGG_KEYS
        i = max((keys.index(k) for k in g_ext), default=-1)
        g = None                    # gradient w.r.t. the output of keys[i] from the layers behind it
        while i >= 0:
            key = keys[i]
            if key[0] == "p":
                rk = keys[i - 1]
                dZ = ops.vgg_pool_act_bwd(g, g_ext.get(key), g_ext.get(rk), saved[rk], avg=self._pool == "avg")
                i, key = i - 1, rk
            else:
                dZ = ops.vgg_act_bwd(g, g_ext.get(key), saved[key], out=g)
            name = arch.VGG_CONV_OF[key]
            if name == "conv1_1":
                w = self.conv1_1.weight
                wt = self._cache.get("vgg_bwd.conv1_1" + (":pre" if preprocess else ""), w,
                                     lambda w: vgg_bwd_weight_conv1(w, preprocess))
                return ops.vgg_conv1_bwd(dZ, wt)
            wt, packs = _bwd_filters(self._cache, "vgg_bwd." + name, getattr(self, name).weight, vgg_bwd_weight)
            g = ops.conv3x3(dZ, wt, packs, None, layer="vgg_bwd." + name)
            del dZ
            i -= 1
        return None

    def _fuses_pool(self, key, i, last, cur, N):
        """Does the convolution behind key `i` (input `cur`) also produce the max pool that follows it?  relu1_2 / relu2_2 /
        relu3_4 / relu4_4 -> pool, when the pool is wanted and the layer goes to the Winograd kernel."""
        name = arch.VGG_CONV_OF[key]
        return (self._pool == "max" and ops.pool_fusion() and i + 1 <= last and key in arch.VGG_POOL_AFTER
                and min(cur.shape[2:]) >= 2
                and ops.winograd_selected(N, cur.shape[1], cur.shape[2], cur.shape[3], getattr(self, name).weight.shape[0],
                                          layer="vgg." + name))

    def _forward(self, x, out_keys, preprocess, _gray, saved=None):
        """The layer walk.  saved: a dict that receives every convolution's post-ReLU output (the full-resolution tensor of a
        pool-fused layer too) — the backward's masks and routes."""
        x = x.detach().float() if _gray else x.detach().contiguous().float()
        N = x.shape[0]
        _check_vgg_keys(out_keys)
        last = max(arch.VGG_KEYS.index(k) for k in out_keys) if out_keys else -1
        out = {}
        cur = x
        pooled = None
        for i, key in enumerate(arch.VGG_KEYS):
            if i > last:
                break  # the reference always runs through p5; the requested outputs are identical
            if key[0] == "p":
                if pooled is not None:          # came out of the convolution in front of it (ops.conv2d_winograd_pool)
                    cur, pooled = pooled, None
                else:
                    cur = ops.maxpool2x2(cur) if self._pool == "max" else ops.avgpool2x2(cur)
            elif self._fuses_pool(key, i, last, cur, N):
                # the pooled tensor comes out of the convolution's own launch; the full-resolution one only when somebody asked
                # for it
                name = arch.VGG_CONV_OF[key]
                conv = getattr(self, name)
                if ops.layer_record is not None:
                    ops.record_layer("vgg." + name, cur.shape[1], conv.weight.shape[0], cur.shape[2], cur.shape[3])
                cur, pooled = ops.conv2d_winograd_pool(cur, _packs(self._cache, name, conv.weight)("winograd"), conv.bias.detach(),
                                                       act=ops.ACT_RELU, want_full=key in out_keys or saved is not None)
            else:
                name = arch.VGG_CONV_OF[key]
                conv = getattr(self, name)
                bias = conv.bias.detach()
                if name == "conv1_1" and preprocess:
                    # vgg_preprocess folded into the load (BGR weight flip + per-channel affine)
                    sc, sh = self._pre_affine(N)
                    cur = ops.conv2d(cur, self._packed(name, swap_bgr=True), bias, act=ops.ACT_RELU,
                                     in_scale=sc, in_shift=sh, gray_input=_gray)
                else:
                    cur = ops.conv3x3(cur, conv.weight, _packs(self._cache, name, conv.weight), bias, act=ops.ACT_RELU,
                                      layer="vgg." + name)
            out[key] = cur
            if saved is not None and key[0] == "r":
                saved[key] = cur
        return [out[key] for key in out_keys]


# ============================================================================================== WarpNet
class _Up4(torch.autograd.Function):
    """x4 nearest upsample (NonlocalNet.py:497-498) with its backward, the 4x4 block sum."""

    @staticmethod
    def forward(ctx, x):
        return ops.upsample_nearest(x.detach().contiguous(), 4)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return ops.warp_up4_bwd(g.contiguous())


class _WarpTrain(torch.autograd.Function):
    """WarpNet behind the trunk tensor — the residual blocks of both sides, the theta / phi projections, centre-and-normalise —
    with what the backward needs saved (WarpNet._trunk_forward_saving); backward returns the gradient of every trunk / projection
    parameter that requires grad and, when a trunk tensor requires grad, the gradient at the seam."""

    @staticmethod
    def forward(ctx, trunkA, trunkB, module, names, *params):
        saved = {}
        theta, phi = module._trunk_forward_saving(trunkA.detach(), trunkB.detach(), saved)
        ctx.module, ctx.names = module, names
        _save_dict(ctx, saved)
        return theta, phi

    @staticmethod
    @once_differentiable
    def backward(ctx, g_theta, g_phi):
        tensors = _saved_dict(ctx)
        need = {n for n, flag in zip(ctx.names, ctx.needs_input_grad[4:]) if flag}
        seam = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dA, dB, grads = ctx.module._trunk_backward(tensors, g_theta, g_phi, need, need_trunk_input_grad=seam)
        return (dA, dB, None, None) + tuple(grads.get(n) for n in ctx.names)


class _WarpHeadsTrain(torch.autograd.Function):
    """WarpNet's four heads on both sides as one batch of 2N (WarpNet._heads_forward_saving), with what their backward needs
    saved; backward takes the seam gradients (dA, dB) that _WarpTrain returns and gives the gradient of every head parameter
    that requires grad (WarpNet._heads_backward).  The feature inputs are data."""

    @staticmethod
    def forward(ctx, module, names, feats, *params):
        N = feats[0].shape[0]
        need = {n for n, flag in zip(names, ctx.needs_input_grad[3:]) if flag}
        saved = {}
        trunk, rpad5 = module._heads_forward_saving([torch.cat((a, b), 0) for a, b in zip(feats[:4], feats[4:])], need, saved)
        ctx.module, ctx.names, ctx.rpad5 = module, names, rpad5
        _save_dict(ctx, saved)
        return trunk[:N], trunk[N:]

    @staticmethod
    @once_differentiable
    def backward(ctx, dA, dB):
        need = {n for n, flag in zip(ctx.names, ctx.needs_input_grad[3:]) if flag}
        grads = ctx.module._heads_backward(_saved_dict(ctx), torch.cat((dA, dB), 0), need, ctx.rpad5)
        return (None, None, None) + tuple(grads.get(n) for n in ctx.names)


class _ResidualBlockParams(nn.Module):
    """Parameter container with the reference's names (conv1, conv2, prelu), NonlocalNet.py:330-339."""

    def __init__(self, ch):
        super().__init__()
        self.conv1 = nn.Conv2d(ch, ch, kernel_size=3, padding=0, stride=1)
        self.conv2 = nn.Conv2d(ch, ch, kernel_size=3, padding=0, stride=1)
        self.prelu = nn.PReLU()


def _head_container(spec):
    n = max(max(ci, pi) for (ci, _, _, _, pi) in spec["convs"]) + 1
    if spec["up_out"]:
        n += 1
    mods = [nn.Identity() for _ in range(n)]
    for (ci, cin, cout, stride, pi) in spec["convs"]:
        mods[ci] = nn.Conv2d(cin, cout, kernel_size=3, padding=0, stride=stride)
        mods[pi] = nn.PReLU()
    return nn.Sequential(*mods)


class WarpNet(nn.Module):
    """ input is Al, Bl, channel = 1, range~[0,255] (docstring of NonlocalNet.py:356) """

    def __init__(self, batch_size):
        super().__init__()
        self.feature_channel = arch.WARP_FEATURE_CH
        self.in_channels = self.feature_channel * 4
        self.inter_channels = arch.WARP_TRUNK_CH
        for name in arch.WARP_HEAD_ORDER:
            setattr(self, name, _head_container(arch.WARP_HEADS[name]))
        self.layer = nn.Sequential(*[_ResidualBlockParams(arch.WARP_TRUNK_CH)
                                     for _ in range(arch.WARP_NUM_RESBLOCKS)])
        self.theta = nn.Conv2d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        self.phi = nn.Conv2d(self.in_channels, self.inter_channels, kernel_size=1, stride=1, padding=0)
        self._cache = _PackCache()
        # "fp32": exact-fp32 MFMA affinities.  "bf16": bf16 MFMA candidate filter + exact fp32 re-scoring
        # (BASELINE configs[4]); exact for temperature <= 1e-4, otherwise the fp32 kernel is used.
        self.corr_precision = "fp32"

    # -- helpers
    def _use_bf16(self, temperature, WTA_scale_weight):
        return self.corr_precision == "bf16" and float(temperature) <= 1e-4 and WTA_scale_weight == 1

    def _pk(self, key, conv):
        return self._cache.get(key, conv.weight, ops.pack_conv_weight)

    def _conv3(self, key, conv, x, **kw):
        return ops.conv3x3(x, conv.weight, _packs(self._cache, key, conv.weight), conv.bias.detach(), layer="warp." + key, **kw)

    def prepare(self):
        """Pack every weight now, on the current stream (see _PackCache.get)."""
        for hd in arch.WARP_HEAD_PLAN:
            for ci in (hd.conv_a, hd.conv_b):
                _prepack(self._cache, f"{hd.name}.{ci}", getattr(self, hd.name)[ci])
        for b in range(arch.WARP_NUM_RESBLOCKS):
            _prepack(self._cache, f"layer.{b}.conv1", self.layer[b].conv1)
            _prepack(self._cache, f"layer.{b}.conv2", self.layer[b].conv2)
        self._pk("theta", self.theta)
        self._pk("phi", self.phi)

    def features(self, r2, r3, r4, r5):
        """Heads + concat + residual trunk for one side (NonlocalNet.py:451-465) -> [N,256,h,w]."""
        return self._trunk(self._heads(r2, r3, r4, r5))

    def _heads(self, r2, r3, r4, r5):
        """The four heads of one side, concatenated: the `trunk` tensor [N,256,h,w] the residual blocks start from."""
        feats = [r2, r3, r4, r5]
        N = r2.shape[0]
        h, w, rpad5 = arch.warp_trunk_geometry([x.shape[2:] for x in feats])
        trunk = torch.empty((N, arch.WARP_TRUNK_CH, h, w), device=r2.device, dtype=torch.float32)
        bs = arch.WARP_TRUNK_CH * h * w
        # The four heads are mutually independent (NonlocalNet.py:451-458): they advance stage by stage — first convolutions,
        # their norms, second convolutions, final norms into the trunk's channel slices — and each stage is ONE launch over the
        # heads that take the same kind of kernel (ops.conv3x3_group / ops.instnorm_apply_group: bit-identical to per-layer
        # launches, which DVC_GROUP_HEADS=0 brings back).  The stride-2 head (layer2_1, run-time-geometry direct kernel with
        # the norm applied on load) keeps its own launches.
        heads = arch.WARP_HEAD_PLAN
        seqs = [getattr(self, hd.name) for hd in heads]

        def conv_item(hd, ci, x, **kw):
            key, conv = f"{hd.name}.{ci}", seqs[hd.index][ci]
            return dict(x=x, weight=conv.weight, packs=_packs(self._cache, key, conv.weight), bias=conv.bias.detach(),
                        layer="warp." + key, pad_mode=ops.PAD_REFLECT, **kw)

        # stage 1: first convolutions
        t1 = ops.conv3x3_group([conv_item(hd, hd.conv_a, feats[hd.index], defer_reduce=hd.stride_b == 1) for hd in heads])
        # stage 2: InstanceNorm + PReLU, materialised (one launch for the four heads, in place where the convolution wrote a
        # tensor) so that the next convolution has no fused input transform.  r06: the stride-2 head too — up to r05 its
        # statistics were a launch of their own and the stride-2 convolution applied them on load; as an item of the grouped
        # launch the norm costs nothing extra, and the convolution (run-time-geometry kernel, register staging either way)
        # reads the normalised tensor
        normed = ops.instnorm_apply_group([dict(x=t, out=None if isinstance(t, ops.ConvPartials) else t,
                                                slope_t=seq[hd.prelu_a].weight.detach()) for hd, seq, t in zip(heads, seqs, t1)])
        t2 = [None] * len(heads)
        for hd, seq in zip(heads, seqs):    # (before the grouped launch: a split-K direct convolution uses the same workspace)
            if hd.stride_b != 1:
                cb = seq[hd.conv_b]
                t2[hd.index] = ops.conv2d(normed[hd.index], self._pk(f"{hd.name}.{hd.conv_b}", cb), cb.bias.detach(),
                                          stride=hd.stride_b, pad_mode=ops.PAD_REFLECT, in_up=2 if hd.up_mid else 1)
        # stage 3: second convolutions
        plain = [hd for hd in heads if hd.stride_b == 1]
        second = ops.conv3x3_group([conv_item(hd, hd.conv_b, normed[hd.index], in_up=2 if hd.up_mid else 1, defer_reduce=True)
                                    for hd in plain])
        for hd, t in zip(plain, second):
            t2[hd.index] = t
        # stage 4: final norms (+ PReLU, x2 upsample, replicated rows) into the trunk's channel slices
        ops.instnorm_apply_group([dict(x=t, slope_t=seq[hd.prelu_b].weight.detach(), up=2 if hd.up_out else 1,
                                       rpad=rpad5 if hd.name == "layer5_1" else 0,
                                       out=trunk[:, hd.index * arch.WARP_FEATURE_CH:(hd.index + 1) * arch.WARP_FEATURE_CH],
                                       out_batch_stride=bs) for hd, seq, t in zip(heads, seqs, t2)])
        return trunk

    def _trunk(self, x, saved=None):
        """The three residual blocks (NonlocalNet.py:341-352,464).  saved: a dict that receives what the backward needs (training
        path) — per block b its input "x{b}", the two InstanceNorm outputs "n1.{b}" / "n2.{b}" with their per-plane 1/sigma
        "rstd1.{b}" / "rstd2.{b}" and the first PReLU's output "p1.{b}".  The split-K reduce is then never deferred into a norm and
        each PReLU is a launch of its own (ops.warp_prelu_fwd: the norm launch's own expression, bit-identical values), so that
        every one of these exists as a tensor."""
        for b in range(arch.WARP_NUM_RESBLOCKS):
            blk = self.layer[b]
            a = blk.prelu.weight.detach()
            if saved is not None:
                planes = x.shape[0] * x.shape[1]
                r1, r2 = (torch.empty(planes, device=x.device, dtype=torch.float32) for _ in range(2))
                t = self._conv3(f"layer.{b}.conv1", blk.conv1, x, pad_mode=ops.PAD_REFLECT)
                n1 = ops.instnorm_apply(t, out=t, scale_out=r1)
                p1 = ops.warp_prelu_fwd(n1, a)
                t = self._conv3(f"layer.{b}.conv2", blk.conv2, p1, pad_mode=ops.PAD_REFLECT)
                n2 = ops.instnorm_apply(t, out=t, scale_out=r2)
                saved.update({f"x{b}": x, f"n1.{b}": n1, f"rstd1.{b}": r1, f"p1.{b}": p1, f"n2.{b}": n2, f"rstd2.{b}": r2})
                x = ops.warp_prelu_fwd(n2, a, skip=x)
                continue
            t = self._conv3(f"layer.{b}.conv1", blk.conv1, x, pad_mode=ops.PAD_REFLECT, defer_reduce=True)
            t = _norm_in_place(t, slope_t=a)
            t = self._conv3(f"layer.{b}.conv2", blk.conv2, t, pad_mode=ops.PAD_REFLECT, defer_reduce=True)
            x = _norm_in_place(t, residual=x, slope_t=a)
        return x

    def project(self, which, feats, bf16=False, saved=None):
        """theta / phi: 1x1 conv, centre over positions, L2-normalise over channels -> [N,256,P]
        (bf16=True: the ([N,P,256] fp32, [N,P,256] bf16) pair the bf16 correlation consumes).  saved: a dict that receives the
        convolution's output "t.<which>" and its per-row means "mean.<which>" (training path, fp32 only)."""
        conv = getattr(self, which)
        t = ops.conv2d(feats, self._pk(which, conv), conv.bias.detach(), ksize=1, pad=0)
        if saved is not None:
            assert not bf16
            out, mean = ops.corr_prepare_with_mean(t)
            saved["t." + which], saved["mean." + which] = t, mean
            return out
        return ops.corr_prepare_bf16(t) if bf16 else ops.corr_prepare(t)

    # ---- the training path (train.py:402-427 trains nonlocal_net jointly with colornet): everything behind the trunk tensor
    _HEADS = tuple(arch.WARP_HEAD_ORDER)

    def _trunk_named_parameters(self):
        """The 19 parameters behind the trunk tensor: layer.*, theta.*, phi.*."""
        return [(n, p) for n, p in self.named_parameters() if n.split(".")[0] in ("layer", "theta", "phi")]

    def _head_named_parameters(self):
        return [(n, p) for n, p in self.named_parameters() if n.split(".")[0] in self._HEADS]

    @property
    def head_training(self):
        """Whether the training path also gives the 24 gradients of the four heads (set_head_training)."""
        return self.__dict__.get("_head_training", False)

    def set_head_training(self, flag=True):
        """Opt in to (or out of) the heads' gradients: with it on, any of the 43 parameters requiring grad opens the training
        path and backward fills every one of them that requires grad; with it off (the default) an unfrozen head is refused.
        Not part of state_dict(); kept by pickling / copy.deepcopy.  Returns self."""
        self.__dict__["_head_training"] = bool(flag)
        return self

    def _takes_training_path(self):
        named = self.named_parameters() if self.head_training else self._trunk_named_parameters()
        return self.training and torch.is_grad_enabled() and any(p.requires_grad for _, p in named)

    def _check_training_call(self, exemplar_cache, return_taps, defer_merge, detach_flag):
        unfrozen = [] if self.head_training else [n for n, p in self._head_named_parameters() if p.requires_grad]
        if unfrozen:
            raise NotImplementedError(
                f"WarpNet: the training path gives the gradients of the residual trunk and the theta / phi projections only "
                f"(layer.*, theta.*, phi.*); {len(unfrozen)} head parameters require grad ({unfrozen[0]}, ...); freeze the heads: "
                "`for head in (net.layer2_1, net.layer3_1, net.layer4_1, net.layer5_1): "
                "[p.requires_grad_(False) for p in head.parameters()]`")
        for flag, what in ((exemplar_cache is not None, "exemplar_cache"), (return_taps, "return_taps"), (defer_merge, "defer_merge"),
                           (detach_flag, "detach_flag=True")):
            if flag:
                raise NotImplementedError(f"WarpNet: `{what}` is not supported on the training path (training mode, grad mode on, "
                                          "a trunk / projection parameter requiring grad); call under torch.no_grad() or .eval()")

    def _forward_with_grad(self, ins, temperature, WTA_scale_weight):
        """(y, similarity_map) bit-identical to the no-grad forward on the fp32 correlation, with a backward to the trunk /
        projection parameters.  The heads run as they do in inference, without history — or, after set_head_training with a head
        parameter requiring grad, with history (_WarpHeadsTrain); the exemplar memo is neither read nor filled."""
        B_lab_map, A2, A3, A4, A5, B2, B3, B4, B5 = ins
        fh, fw = int(B_lab_map.shape[2] / 4), int(B_lab_map.shape[3] / 4)
        heads = self._head_named_parameters() if self.head_training else []
        _check_trainable(self._trunk_named_parameters() + heads, "WarpNet")
        with torch.no_grad():
            blab = ops.avgpool4x4(B_lab_map)
        if any(p.requires_grad for _, p in heads):
            # set_head_training: the heads run with history too, layer by layer, both sides as one batch
            trunkA, trunkB = _WarpHeadsTrain.apply(self, tuple(n for n, _ in heads), tuple(ins[1:]), *(p for _, p in heads))
        else:
            with torch.no_grad():
                trunkA = self._heads(A2, A3, A4, A5)
                trunkB = self._heads(B2, B3, B4, B5)
        if (trunkA.shape[2], trunkA.shape[3]) != (fh, fw):
            raise RuntimeError(f"shape '[{B_lab_map.shape[0]}, 1, {fh}, {fw}]' is invalid for feature map "
                               f"of size {tuple(trunkA.shape[2:])}")
        return self._train_from_trunks(trunkA, trunkB, blab, temperature, WTA_scale_weight)

    def _train_from_trunks(self, trunkA, trunkB, blab, temperature, WTA_scale_weight=1):
        """The differentiable part: trunk tensors [N,256,h,w] of both sides -> (y, similarity_map).  A trunk tensor that requires
        grad gets its gradient too — the seam the heads' backward will start from (need_trunk_input_grad of _trunk_backward)."""
        from .corr_autograd import fused_correlation
        N, _, fh, fw = trunkA.shape
        named = self._trunk_named_parameters()
        theta, phi = _WarpTrain.apply(trunkA, trunkB, self, tuple(n for n, _ in named), *(p for _, p in named))
        y, sim, _ = fused_correlation(theta, phi, blab.view(N, 3, -1), float(temperature), fh, fw, WTA_scale_weight)
        return _Up4.apply(y), _Up4.apply(sim)

    def _trunk_forward_saving(self, trunkA, trunkB, saved):
        """Both sides as one batch of 2N images through the shared blocks, then theta on the A half and phi on the B half."""
        N = trunkA.shape[0]
        F = self._trunk(torch.cat((trunkA, trunkB), 0), saved=saved)
        saved["F"] = F
        return self.project("theta", F[:N], saved=saved), self.project("phi", F[N:], saved=saved)

    def _trunk_backward(self, t, g_theta, g_phi, need, need_trunk_input_grad=False):
        """Parameter gradients (names in `need`) from the saved tensors `t` (WarpNet._trunk(saved=...), project(saved=...)) and the
        gradients at the centred, normalised theta / phi [N,256,P].  need_trunk_input_grad: also the gradient at the trunk
        tensor of both sides, (dA, dB) — the seam; a normal training step skips that convolution.  Returns (dA, dB, grads)."""
        grads = {}
        F = t["F"]
        M, C, h, w = F.shape
        N = M // 2
        dF = torch.empty_like(F)
        need_blocks = need_trunk_input_grad or any(n.startswith("layer.") for n in need)
        for which, g, sl in (("theta", g_theta, slice(0, N)), ("phi", g_phi, slice(N, M))):
            conv = getattr(self, which)
            dt = ops.warp_cn_bwd(t["t." + which], t["mean." + which], g.contiguous())
            if _wants(need, which):
                _put_wb(grads, need, which, *ops.warp_k1_wgrad(dt, F[sl]))
            if need_blocks:
                wt = self._cache.get("warp_bwd." + which, conv.weight,
                                     lambda w: ops.pack_conv_weight(w.detach().transpose(0, 1).contiguous()))
                ops.conv2d(dt.view(N, -1, h, w), wt, None, ksize=1, pad=0, out=dF[sl])
        if not need_blocks:
            return None, None, grads
        g = dF
        for b in reversed(range(arch.WARP_NUM_RESBLOCKS)):
            blk = self.layer[b]
            a = blk.prelu.weight.detach()
            c1, c2 = f"layer.{b}.conv1", f"layer.{b}.conv2"
            sp = torch.empty((2, M * C), device=F.device, dtype=torch.float64)
            # second site: out = prelu(n2 + x)
            dz, du, _ = ops.warp_norm_prelu_bwd(g, t[f"n2.{b}"], t[f"rstd2.{b}"], a, skip=t[f"x{b}"], slope_part=sp[0])
            if _wants(need, c2):
                _put_wb(grads, need, c2, *ops.cvn_wgrad(dz, ops.warp_reflect_pad(t[f"p1.{b}"])))
            wt, packs = _bwd_filters(self._cache, "warp_bwd." + c2, blk.conv2.weight, vgg_bwd_weight)
            gp = ops.conv3x3(dz, wt, packs, None, layer="warp_bwd." + c2)
            g = ops.warp_fold(gp)
            del gp, dz
            # first site: p1 = prelu(n1)
            dz, _, _ = ops.warp_norm_prelu_bwd(g, t[f"n1.{b}"], t[f"rstd1.{b}"], a, slope_part=sp[1])
            if _wants(need, c1):
                _put_wb(grads, need, c1, *ops.cvn_wgrad(dz, ops.warp_reflect_pad(t[f"x{b}"])))
            if f"layer.{b}.prelu.weight" in need:
                grads[f"layer.{b}.prelu.weight"] = ops.warp_slope_sum(sp)
            if b == 0 and not need_trunk_input_grad:
                return None, None, grads
            wt, packs = _bwd_filters(self._cache, "warp_bwd." + c1, blk.conv1.weight, vgg_bwd_weight)
            gp = ops.conv3x3(dz, wt, packs, None, layer="warp_bwd." + c1)
            g = ops.warp_fold(gp, skip=du)
            del gp, dz, du
        return g[:N], g[N:], grads

    # ---- the heads with history (set_head_training): arch.WARP_HEAD_PLAN walked layer by layer, forward and backward
    def _heads_forward_saving(self, feats, need, saved):
        """The four heads on `feats` (relu2_1 .. relu5_1 of both sides as one batch) -> (the trunk tensor [2N,256,h,w], rpad5).
        A head with a parameter in `need` runs site by site — conv, InstanceNorm, PReLU as launches of their own, the values of
        the fused launches of _heads bit for bit (see _trunk) — and leaves in `saved`, under "<head>." + key: its input "x" and per
        site the norm output "na" / "nb", its 1/sigma "ra" / "rb" and the first PReLU's output "pa".  Any other head keeps the
        fused norm launches and saves nothing."""
        M = feats[0].shape[0]
        h, w, rpad5 = arch.warp_trunk_geometry([x.shape[2:] for x in feats])
        trunk = torch.empty((M, arch.WARP_TRUNK_CH, h, w), device=feats[0].device, dtype=torch.float32)
        bs = arch.WARP_TRUNK_CH * h * w

        def stat(t):
            return torch.empty(t.shape[0] * t.shape[1], device=t.device, dtype=torch.float32)

        for hd in arch.WARP_HEAD_PLAN:
            seq = getattr(self, hd.name)
            ca, cb = seq[hd.conv_a], seq[hd.conv_b]
            slope_a, slope_b = seq[hd.prelu_a].weight.detach(), seq[hd.prelu_b].weight.detach()
            keep = any(n.startswith(hd.name + ".") for n in need)
            rpad = rpad5 if hd.name == "layer5_1" else 0
            out = trunk[:, hd.index * arch.WARP_FEATURE_CH:(hd.index + 1) * arch.WARP_FEATURE_CH]
            x = feats[hd.index]
            t = self._conv3(f"{hd.name}.{hd.conv_a}", ca, x, pad_mode=ops.PAD_REFLECT)
            if keep:
                ra = stat(t)
                na = ops.instnorm_apply(t, out=t, scale_out=ra)
                pa = ops.warp_prelu_fwd(na, slope_a)
            else:
                pa = ops.instnorm_apply(t, out=t, slope_t=slope_a)
            in_up = 2 if hd.up_mid else 1
            if hd.stride_b != 1:
                t = ops.conv2d(pa, self._pk(f"{hd.name}.{hd.conv_b}", cb), cb.bias.detach(), stride=hd.stride_b,
                               pad_mode=ops.PAD_REFLECT, in_up=in_up)
            else:
                t = self._conv3(f"{hd.name}.{hd.conv_b}", cb, pa, pad_mode=ops.PAD_REFLECT, in_up=in_up)
            if not keep:
                ops.instnorm_apply(t, slope_t=slope_b, up=2 if hd.up_out else 1, rpad=rpad, out=out, out_batch_stride=bs)
                continue
            rb = stat(t)
            nb = ops.instnorm_apply(t, out=t, scale_out=rb)
            pb = ops.warp_prelu_fwd(nb, slope_b)
            if hd.up_out:
                pb = ops.upsample_nearest(pb, 2)
            out[:, :, rpad:h - rpad].copy_(pb)
            if rpad:
                out[:, :, :rpad].copy_(pb[:, :, :1])
                out[:, :, h - rpad:].copy_(pb[:, :, -1:])
            saved.update({f"{hd.name}.x": x, f"{hd.name}.na": na, f"{hd.name}.ra": ra, f"{hd.name}.pa": pa,
                          f"{hd.name}.nb": nb, f"{hd.name}.rb": rb})
        return trunk, rpad5

    def _heads_backward(self, t, g_trunk, need, rpad5):
        """Head parameter gradients (names in `need`) from the saved tensors `t` (_heads_forward_saving) and the gradient at
        the trunk tensor of both sides g_trunk [2N,256,h,w].  Per head: its channel slice, the adjoints of the replicated rows and
        of the x2 upsample, the second site's norm + PReLU backward, that convolution's weight gradient (dvc_warp_head_wgrad:
        every head convolution, stride 1 or 2) and input gradient (W^T flipped on the forward's engines, a stride-2 layer's dz
        spread by dvc_warp_dilate_ring first, then the fold), the adjoint of the inner upsample, the first site, the first
        convolution's weight gradient.  The first convolution's input is data: no gradient.  A head with nothing in `need` is
        skipped, and a head stops where nothing in front of it is wanted."""
        grads = {}
        for hd in arch.WARP_HEAD_PLAN:
            pre = hd.name + "."
            if not any(n.startswith(pre) for n in need):
                continue
            seq = getattr(self, hd.name)
            ka, kb = f"{pre}{hd.conv_a}", f"{pre}{hd.conv_b}"
            sa, sb = f"{pre}{hd.prelu_a}.weight", f"{pre}{hd.prelu_b}.weight"
            g = g_trunk[:, hd.index * arch.WARP_FEATURE_CH:(hd.index + 1) * arch.WARP_FEATURE_CH].contiguous()
            if hd.name == "layer5_1" and rpad5:
                g = ops.warp_rpad_rows_bwd(g, rpad5)
            if hd.up_out:
                g = ops.warp_up2_bwd(g)
            dz, _, sp = ops.warp_norm_prelu_bwd(g, t[pre + "nb"], t[pre + "rb"], seq[hd.prelu_b].weight.detach())
            if sb in need:
                grads[sb] = ops.warp_slope_sum(sp)
            xb = ops.upsample_nearest(t[pre + "pa"], 2) if hd.up_mid else t[pre + "pa"]
            if _wants(need, kb):
                _put_wb(grads, need, kb, *ops.warp_head_wgrad(dz, ops.warp_reflect_pad(xb), stride=hd.stride_b))
            if not (_wants(need, ka) or sa in need):
                continue
            if hd.stride_b == 2:
                dz = ops.warp_dilate_ring(dz, xb.shape[2], xb.shape[3])
            wt, packs = _bwd_filters(self._cache, "warp_bwd." + kb, seq[hd.conv_b].weight, vgg_bwd_weight)
            g = ops.warp_fold(ops.conv3x3(dz, wt, packs, None, layer="warp_bwd." + kb))
            del dz, xb
            if hd.up_mid:
                g = ops.warp_up2_bwd(g)
            dz, _, sp = ops.warp_norm_prelu_bwd(g, t[pre + "na"], t[pre + "ra"], seq[hd.prelu_a].weight.detach())
            if sa in need:
                grads[sa] = ops.warp_slope_sum(sp)
            if _wants(need, ka):
                _put_wb(grads, need, ka, *ops.warp_head_wgrad(dz, ops.warp_reflect_pad(t[pre + "x"])))
        return grads

    # ---- transparent exemplar memo (r05).  The reference's loop (test.py:68-96) hands the SAME exemplar tensors to every
    # frame_colorization call and NonlocalNet.py:452-465,473-476,491-493 recompute the exemplar side each time.  A caller that is
    # not rewritten around ClipColorizer gets the cached form anyway: the exemplar side is memoised on the identity and the
    # version counters of the tensors it was computed from (the memo holds references to them, so their addresses cannot be
    # recycled for other data while it is alive), this module's parameters (data_ptr, _version) and everything that selects
    # kernels.  An in-place write to a key tensor bumps its `_version` and misses.  What no version counter sees:
    #   * tensors created under torch.inference_mode() have no version counter at all — the memo is bypassed for them (the
    #     exemplar side is recomputed per call, as the reference does);
    #   * writes through `.data` (`t.data.copy_(...)`, `p.data.mul_(...)`) are invisible here as they are to autograd: NOT
    #     supported with the memo on.  DVC_EXEMPLAR_MEMO=verify / ops.set_exemplar_memo("verify")
    #     recomputes on every hit, compares bit for bit, warns on a mismatch and returns the fresh value.
    # DVC_EXEMPLAR_MEMO=0 / ops.set_exemplar_memo(False) turns the memo off.
    def _memo_exemplar_side(self, key_tensors, regime, compute):
        mode = ops.exemplar_memo_mode()
        if mode == "off":
            return compute()
        versions = [_version_of(t) for t in key_tensors]
        pfp = tuple((p.data_ptr(), _version_of(p)) for p in self.parameters())
        if any(v is None for v in versions) or any(v is None for _, v in pfp):
            return compute()        # inference tensors: nothing to key a change on
        fp = (pfp, regime, ops.conv_algo(), ops.direct_layers(), ops.fuse_reduce(), ops.autotune_enabled(),
              ops.batch_plan_enabled(), ops.group_heads(), ops.ws_conv_enabled())
        memo = getattr(self, "_exemplar_memo", None)
        if (memo is not None and memo[1] == fp and len(memo[0]) == len(key_tensors)
                and all(a is b and va == vb for (a, va), b, vb in zip(memo[0], key_tensors, versions))):
            if mode != "verify":
                return memo[2]
            fresh = compute()
            if _same_tensors(fresh, memo[2]):
                return memo[2]
            import warnings
            warnings.warn("DVC_EXEMPLAR_MEMO=verify: the memoised exemplar side differs from a recomputation although no key "
                          "tensor or WarpNet parameter changed identity or version — something wrote to them through `.data` "
                          "(unsupported with the memo on); using the recomputed value", RuntimeWarning, stacklevel=3)
            value = fresh
        else:
            value = compute()
        # (object.__setattr__: the memo holds tensors, nn.Module.__setattr__ would try to register them)
        object.__setattr__(self, "_exemplar_memo", ([(t, v) for t, v in zip(key_tensors, versions)], fp, value))
        return value

    def __getstate__(self):
        # (pickling / copy.deepcopy of the module: the memo is a cache of tensors, not state)
        state = dict(self.__dict__)
        state.pop("_exemplar_memo", None)
        return state

    def exemplar_side(self, B_lab_map, B2, B3, B4, B5, bf16=None):
        """Everything that depends only on the exemplar (recomputed per frame by the reference,
        NonlocalNet.py:452-465,473-476,491-493; cacheable per clip)."""
        if bf16 is None:
            bf16 = self.corr_precision == "bf16"
        phi = self.project("phi", self.features(B2, B3, B4, B5), bf16=bf16)
        blab = ops.avgpool4x4(B_lab_map)
        return phi, blab

    def forward(self, B_lab_map, A_relu2_1, A_relu3_1, A_relu4_1, A_relu5_1, B_relu2_1, B_relu3_1,
                B_relu4_1, B_relu5_1, temperature=0.001 * 5, detach_flag=False, WTA_scale_weight=1,
                feature_noise=0, exemplar_cache=None, return_taps=False, defer_merge=False):
        """models/NonlocalNet.py:427-502 -> (y, similarity_map).  Not upstream: `exemplar_cache` (the exemplar side computed once
        per clip), `return_taps`, and `defer_merge` — the fp32 correlation then leaves the merge of its partial softmax states
        to the consumer and the call returns (ops.CorrPartials, None) for ops.pack_color_input (dvc_amd/frame.py)."""
        ins = [B_lab_map, A_relu2_1, A_relu3_1, A_relu4_1, A_relu5_1, B_relu2_1, B_relu3_1, B_relu4_1,
               B_relu5_1]
        for t in ins:
            _check_input(t, "WarpNet")
        if self._takes_training_path():
            self._check_training_call(exemplar_cache, return_taps, defer_merge, detach_flag)
            return self._forward_with_grad([t.detach().contiguous().float() for t in ins], temperature, WTA_scale_weight)
        memo_key = (B_lab_map, B_relu2_1, B_relu3_1, B_relu4_1, B_relu5_1)      # (the caller's own tensor objects)
        ins = [t.detach().contiguous().float() for t in ins]
        B_lab_map, A2, A3, A4, A5, B2, B3, B4, B5 = ins
        image_height, image_width = B_lab_map.shape[2], B_lab_map.shape[3]
        fh, fw = int(image_height / 4), int(image_width / 4)
        A_features = self.features(A2, A3, A4, A5)
        if (A_features.shape[2], A_features.shape[3]) != (fh, fw):
            raise RuntimeError(f"shape '[{B_lab_map.shape[0]}, 1, {fh}, {fw}]' is invalid for feature map "
                               f"of size {tuple(A_features.shape[2:])}")
        bf16 = self._use_bf16(temperature, WTA_scale_weight)
        if exemplar_cache is not None:
            phi, blab = exemplar_cache
            if isinstance(phi, tuple) != bf16:
                raise RuntimeError("exemplar cache was built for a different corr_precision / temperature regime")
        else:
            phi, blab = self._memo_exemplar_side(memo_key, ("forward", bf16),
                                                 lambda: self.exemplar_side(B_lab_map, B2, B3, B4, B5, bf16=bf16))
        theta = self.project("theta", A_features, bf16=bf16)
        if bf16:
            res = ops.corr_fwd_bf16(theta, phi, blab.view(blab.shape[0], 3, -1), float(temperature), fh, fw,
                                    want_small=return_taps, want_argmax=return_taps)
        else:
            res = ops.corr_fwd(theta, phi, blab.view(blab.shape[0], 3, -1), float(temperature), fh, fw,
                               wta_scale=float(WTA_scale_weight), want_small=return_taps,
                               want_argmax=return_taps, defer_merge=defer_merge and not return_taps)
            if isinstance(res, ops.CorrPartials):
                return res, None
        if return_taps:
            return res["y_up"], res["sim_up"], dict(theta=theta, phi=phi, y_small=res["y_small"],
                                                    sim_small=res["sim_small"], argmax=res["argmax"],
                                                    A_features=A_features)
        return res["y_up"], res["sim_up"]


# ========================================================================================== ColorVidNet
def cvn_bwd_weight(w, pad_to=None):
    """The input-gradient filters of one of ColorVidNet's 3x3 layers (pad == dil, stride 1): W^T flipped, [Cin][Cout][3][3],
    with dilation d the same convolution at dilation d.  pad_to: zero output channels appended up to that count (conv1_1.0's
    7-channel input gradient runs as a 32-channel convolution whose first 7 channels are kept)."""
    wt = vgg_bwd_weight(w)
    if pad_to is not None and wt.shape[0] < pad_to:
        wt = torch.cat((wt, wt.new_zeros((pad_to - wt.shape[0],) + tuple(wt.shape[1:]))), dim=0).contiguous()
    return wt


class _CVNTrain(torch.autograd.Function):
    """ColorVidNet.forward with what the backward needs saved (ColorVidNet._forward(saved=...)); backward walks the layers in
    reverse and returns d x (when x requires grad) and the gradient of every parameter that requires grad."""

    @staticmethod
    def forward(ctx, x, module, names, *params):
        saved, rstd = {}, {}
        ab = module._forward(x, saved=saved, rstd=rstd)
        saved["ab"] = ab
        saved.update(("rstd:" + k, v) for k, v in rstd.items())
        ctx.module, ctx.names = module, names
        _save_dict(ctx, saved)
        return ab

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ab):
        tensors = _saved_dict(ctx)
        need = {n for n, flag in zip(ctx.names, ctx.needs_input_grad[3:]) if flag}
        dx, grads = ctx.module._backward(tensors, g_ab.contiguous(), need, ctx.needs_input_grad[0])
        return (dx, None, None) + tuple(grads.get(n) for n in ctx.names)


class ColorVidNet(nn.Module):
    def __init__(self, ic):
        super().__init__()
        shapes = arch.colorvidnet_param_shapes(ic)
        made = {}
        for key, kind in arch.CVN_STATE_ORDER:
            w = shapes[key + ".weight"]
            if kind == "ss":
                mod = nn.Conv2d(w[0], w[0], 1, 2, bias=False, groups=w[0])
            else:
                k = w[2]
                mod = nn.Conv2d(w[1], w[0], k, 1, 0)
            made[key] = mod
        # group "a.b" keys into Sequential containers so that state_dict keys match the reference
        groups = {}
        for key, mod in made.items():
            if "." in key:
                top, idx = key.split(".")
                groups.setdefault(top, {})[int(idx)] = mod
            else:
                setattr(self, key, mod)
        for top, items in groups.items():
            seq = [nn.Identity() for _ in range(max(items) + 1)]
            for i, m in items.items():
                seq[i] = m
            setattr(self, top, nn.Sequential(*seq))
        # keep the reference's registration order (ColorVidNet.py:9-47) for state_dict()
        order = []
        for key, _ in arch.CVN_STATE_ORDER:
            top = key.split(".")[0]
            if top not in order:
                order.append(top)
        self._modules = type(self._modules)((k, self._modules[k]) for k in order)
        self._ic = ic
        self._cache = _PackCache()
        # the reference constructor prints these two lines (ColorVidNet.py:80,85)
        print("replace all deconv with [nearest + conv]")
        print("replace all batchnorm with instancenorm")

    def _mod(self, key):
        m = self
        for part in key.split("."):
            m = m[int(part)] if part.isdigit() else getattr(m, part)
        return m

    def _ss_weight(self, key):
        return self._cache.get(key, self._mod(key).weight, lambda w: w.detach().reshape(-1).contiguous())

    def _out_weight(self):
        out = self._mod(arch.CVN_OUT["key"])
        return self._cache.get("conv10_ab", out.weight, lambda w: w.detach().reshape(w.shape[0], -1).contiguous())

    # ---- decoder blocks: `conv8_1(up(norm(c7_3))) + conv3_3_short(norm(c3_3))` (ColorVidNet.py:124-127; likewise conv9_1,
    # conv10_1) as ONE launch over the channels of both inputs (ops.conv2d_winograd_dual) when both are Winograd layers.  Which
    # pairs qualify is arch.CVN_GRAPH.dual; _dual_ok adds what only a call knows (switches, shapes, the engine choice)
    def _dual_pack(self, cA, cB):
        """(concatenated Winograd filters, summed bias) of a fused pair; cached per parameter versions like every pack."""
        mA, mB = self._mod(cA["key"]), self._mod(cB["key"])
        u = self._cache.get(cA["key"] + ":dual", (mA.weight, mB.weight), lambda ws: torch.cat(
            (ops.pack_winograd_weight(ws[0]), ops.pack_winograd_weight(ws[1])), dim=1).contiguous())
        b = self._cache.get(cA["key"] + ":dualbias", (mA.bias, mB.bias), lambda bs: (bs[0].detach() + bs[1].detach()).contiguous())
        return u, b

    def _dual_ok(self, cA, cB, shapeA, shapeB):
        """Both convolutions of the pair go to the Winograd kernel under the current algorithm choice."""
        if not ops.dual_conv_enabled():
            return False
        (N, CA, HA, WA), (_, CB, HB, WB) = shapeA, shapeB
        upA = 2 if cA["pre"] == "up" else 1
        # (dvc_conv2d_winograd_dual forces the 64-channel x 32-tile workgroup shape and stages 8-channel chunks of each input)
        if cA["cout"] % 64 or cB["cout"] != cA["cout"] or CA % 8 or CB % 8:
            return False
        return (ops.winograd_selected(N, CA, HA, WA, cA["cout"], dil=cA["dil"], pad=cA["dil"], in_up=upA, layer="cvn." + cA["key"])
                and ops.winograd_selected(N, CB, HB, WB, cB["cout"], dil=cB["dil"], pad=cB["dil"], layer="cvn." + cB["key"]))

    def prepare(self):
        """Pack every weight now, on the current stream (see _PackCache.get)."""
        for c in arch.CVN_CONVS:
            _prepack(self._cache, c["key"], self._mod(c["key"]))
            if c["pre"] == "norm_ss":
                self._ss_weight(c["ss"])
        self._out_weight()
        if ops.conv_algo() != "direct" and ops.dual_conv_enabled():
            G = arch.CVN_GRAPH
            for key, skip in G.dual.items():
                self._dual_pack(G.by_key[key], G.by_key[skip])

    def forward(self, x):
        """ x: gray image (1 channel), ab(2 channel), ab_err, ba_err"""
        if self.training and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return self._forward_with_grad(x)
        _check_input(x, "ColorVidNet")
        return self._forward(x)

    def _forward_with_grad(self, x):
        """The training path (train.py: `colornet.train()`): output bit-identical to the no-grad forward, with a backward to every
        parameter and to x."""
        if not x.is_cuda:
            _check_input(x, "ColorVidNet")
        if x.dtype != torch.float32:
            raise TypeError(f"ColorVidNet: the training path takes a float32 input (got {x.dtype})")
        named = list(self.named_parameters())
        _check_trainable(named, "ColorVidNet")
        return _CVNTrain.apply(x, self, tuple(n for n, _ in named), *(p for _, p in named))

    def _bwd_filters(self, key, pad_to=None):
        """(filters, packs) of the input gradient of the 3x3 layer `key` (cvn_bwd_weight), under "cvn_bwd." keys."""
        return _bwd_filters(self._cache, "cvn_bwd." + key, self._mod(key).weight, lambda w: cvn_bwd_weight(w, pad_to))

    def _backward(self, t, g_ab, need, need_dx):
        """Parameter gradients (names in `need`) and d x (need_dx) from the saved tensors `t` (ColorVidNet._forward(saved=...)):
        the head on dvc_cvn_head_bwd, then CVN_CONVS in reverse — each layer's dZ (ReLU backward, or the InstanceNorm backward
        that gathers the norm's consumers), its weight gradient on dvc_cvn_wgrad, its input gradient on the forward's engines
        with W^T flipped (ops.conv3x3)."""
        G = arch.CVN_GRAPH
        grads = {}
        dZ, dW, db = ops.cvn_head_bwd(t["ab"], g_ab, self._out_weight(), t[arch.CVN_OUT["src"]], slope=0.2)
        _put_wb(grads, need, arch.CVN_OUT["key"], dW, db)
        dZ_of = {arch.CVN_OUT["src"]: dZ}
        contrib = {}                    # activation -> {kind: gradient}
        dx = None
        for c in reversed(arch.CVN_CONVS):
            key, dst, src, pre = c["key"], c["dst"], c["src"], c["pre"]
            if dst in dZ_of:
                dZ = dZ_of[dst]
            elif dst in G.adder:        # a skip convolution (no activation): the dZ of the block it adds into
                dZ = dZ_of[G.adder[dst]]
            else:
                g = contrib.pop(dst)
                if "raw" in g:
                    dZ = ops.vgg_act_bwd(g["raw"], None, t[dst], out=g["raw"])
                else:
                    ss_key = G.ss_of.get(dst)
                    dZ, dss = ops.cvn_inorm_bwd(t["n:" + dst], t["rstd:" + dst], t[dst], g_full=g.get("full"), g_ss=g.get("ss"),
                                                ss_w=self._ss_weight(ss_key) if ss_key else None, g_up=g.get("up"))
                    if dss is not None and ss_key + ".weight" in need:
                        grads[ss_key + ".weight"] = dss.view(-1, 1, 1, 1)
                dZ_of[dst] = dZ
            X = t[src] if pre is None else t["nss:" + src] if pre == "norm_ss" else t["n:" + src]
            in_up = 2 if pre == "up" else 1
            if _wants(need, key):
                _put_wb(grads, need, key, *ops.cvn_wgrad(dZ, X, dil=c["dil"], in_up=in_up))
            if src == "x":
                if need_dx:
                    cin = self._mod(key).weight.shape[1]
                    wt, packs = self._bwd_filters(key, pad_to=max(32, -(-cin // 32) * 32))
                    dx = ops.conv3x3(dZ, wt, packs, None, dil=c["dil"], layer="cvn_bwd." + key)[:, :cin]
                continue
            wt, packs = self._bwd_filters(key)
            gi = ops.conv3x3(dZ, wt, packs, None, dil=c["dil"], layer="cvn_bwd." + key)
            kind = G.grad_kind[pre]
            assert kind not in contrib.get(src, {}), (src, kind)
            contrib.setdefault(src, {})[kind] = gi
        return dx, grads

    def _forward(self, x, saved=None, rstd=None):
        """The layer walk.  saved / rstd: dicts that receive what the backward needs (training path): every convolution's
        post-activation output under its name, each InstanceNorm output under "n:" + source (the scaled stride-2 one under
        "nss:" + source) and its per-plane 1/sigma in `rstd`.  The split-K reduce is then never deferred into a norm's launch
        (bit-identical either way), so that every activation exists as a tensor."""
        x = x.detach().contiguous().float()
        G = arch.CVN_GRAPH
        acts = {"x": x}
        normed = {}
        ss_weight = self._ss_weight

        def rstd_buf(src, ss_key=None):
            if saved is None:
                return None
            assert ss_key is None       # (the plane scale is rstd only without a channel scale)
            a = acts[src]
            rstd[src] = torch.empty(a.shape[0] * a.shape[1], device=a.device, dtype=torch.float32)
            return rstd[src]

        def norm_of(src, ss_key=None):
            """InstanceNorm2d(src) [* the depthwise `_ss` weight, stride 2] as a tensor (ColorVidNet.py:85-94,12).  An
            activation of G.norm_pair (skip convolution: plain; next block: * `_ss` weight, stride 2) gets both tensors from
            one launch."""
            k = (src, ss_key)
            if k not in normed:
                pair = G.norm_pair.get(src)
                if pair is not None:
                    normed[(src, None)], normed[(src, pair)] = ops.instnorm_apply(
                        acts[src], eps=1e-5, second=(ss_weight(pair), 2), scale_out=rstd_buf(src))
                else:
                    normed[k] = ops.instnorm_apply(acts[src], eps=1e-5,
                                                   chan_scale=ss_weight(ss_key) if ss_key else None,
                                                   sub=2 if ss_key else 1, scale_out=rstd_buf(src, ss_key))
                if saved is not None:
                    for (s_, k_), v in normed.items():
                        if s_ == src:
                            saved[("nss:" if k_ else "n:") + src] = v
            return normed[k]

        def produced(dst):
            """Right after `dst` exists: the norms its consumers read (for G.norm_only that launch also adds up the split-K
            partial sums the convolution left)."""
            for ss_key in G.norm_variants.get(dst, ()):
                norm_of(dst, ss_key)

        act_map = {"relu": ops.ACT_RELU, "none": ops.ACT_NONE, "leaky": ops.ACT_LEAKY}
        for c in arch.CVN_CONVS:
            if c["key"] in G.skip_keys:
                continue            # the skip convolution of a decoder block: runs with its consumer below (or just before it)
            e = G.by_key.get(G.dual.get(c["key"]))
            if e is not None:
                srcA = norm_of(c["src"]) if c["pre"] in ("norm", "up") else acts[c["src"]]
                srcB = norm_of(e["src"]) if e["pre"] == "norm" else acts[e["src"]]
                if self._dual_ok(c, e, srcA.shape, srcB.shape):
                    u, b = self._dual_pack(c, e)
                    if ops.layer_record is not None:
                        for cc_, src_ in ((c, srcA), (e, srcB)):
                            ops.record_layer("cvn." + cc_["key"], src_.shape[1], cc_["cout"], src_.shape[2], src_.shape[3], dil=cc_["dil"],
                                             in_up=2 if cc_["pre"] == "up" else 1, dual=c["key"])
                    acts[c["dst"]] = ops.conv2d_winograd_dual(srcA, srcB, u, b, dil=c["dil"], in_upA=2 if c["pre"] == "up" else 1,
                                                              act=act_map[c["act"]], act_slope=0.2)
                    produced(c["dst"])
                    continue
                # not both Winograd layers (direct algorithm, tiny maps): the skip convolution as its own launch, then the adder
                convE = self._mod(e["key"])
                acts[e["dst"]] = ops.conv3x3(srcB, convE.weight, _packs(self._cache, e["key"], convE.weight), convE.bias.detach(),
                                             dil=e["dil"], act=act_map[e["act"]], act_slope=0.2, layer="cvn." + e["key"])
            conv = self._mod(c["key"])
            kw = dict(dil=c["dil"], act=act_map[c["act"]], act_slope=0.2)
            pre = c["pre"]
            src = acts[c["src"]]
            if pre == "norm":
                src = norm_of(c["src"])
            elif pre == "norm_ss":
                src = norm_of(c["src"], c["ss"])
            elif pre == "up":
                src = norm_of(c["src"])
                kw["in_up"] = 2
            if c["add"] is not None:
                kw["residual"] = acts[c["add"]]
            dst = c["dst"]
            acts[dst] = ops.conv3x3(src, conv.weight, _packs(self._cache, c["key"], conv.weight), conv.bias.detach(),
                                    defer_reduce=dst in G.norm_only and saved is None, layer="cvn." + c["key"], **kw)
            produced(dst)
        out = self._mod(arch.CVN_OUT["key"])
        if saved is not None:
            saved.update((a, acts[a]) for a in G.saved_acts)
            saved["x"] = x
        return ops.conv1x1_small(acts[arch.CVN_OUT["src"]], self._out_weight(), out.bias.detach(), act=ops.ACT_TANH128)
