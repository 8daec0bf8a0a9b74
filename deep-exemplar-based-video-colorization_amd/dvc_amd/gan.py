"""Discriminator_x64 (models/GAN_models.py:104-157, models/spectral_normalization.py) on the kernels of csrc/gan.hip and
csrc/gan_wgrad.hip: the forward, the gradient back to the input — what the generator's adversarial term needs (train.py builds
`discriminator(torch.cat(...))` on the generated frames and back-propagates into the generator) — and, after
`set_parameter_training()`, the gradients of its own 21 parameters, the gradient through sigma among them — what train.py's
discriminator step needs.

    from dvc_amd.gan import Discriminator_x64        # instead of `from models.GAN_models import Discriminator_x64`

Same constructor, the same state_dict keys and the same `(output, feature4)` return value as the reference; every forward runs
one power step per SpectralNorm module and updates weight_u / weight_v in place, in train() and in eval(), as the reference
does.

Gradient contract.  By default the module is a frozen critic, as for WarpNet's heads: with every parameter frozen, grad mode on and
an input that requires grad, both outputs are differentiable and their backward fills the input gradient only; a parameter that
requires grad under grad mode is refused.  `discriminator.set_parameter_training()` opts in (per module, not in state_dict()):
then backward also fills every parameter that requires grad, through autograd (so `.grad` accumulates as usual), and the input
gradient only if the input requires grad.  Either way the values are bit-identical to the no-grad forward from the same u / v
state.  The sigma of a layer is u'^T W_bar v' with the vectors u', v' that THIS forward's power step left; the training path keeps
its own copies of them per forward, so two forwards followed by one backward (train.py's discriminator step) differentiate each
forward through its own sigma.  Launch sequence and where the LeakyReLU masks sit: DESIGN.md, "Discriminator_x64".
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import arch, ops

SLOPE = arch.GAN_LRELU_SLOPE


def _l2normalize(v, eps=arch.GAN_SN_EPS):
    return v / (v.norm() + eps)


class SpectralNorm(nn.Module):
    """Parameter container with the reference's names: module.bias, module.weight_u, module.weight_v, module.weight_bar
    (spectral_normalization.py:11-53).  `sigma_step()` is the reference's `_update_u_v` with one power iteration."""

    def __init__(self, module):
        super().__init__()
        self.module = module
        w = module.weight
        height = w.shape[0]
        width = w.numel() // height
        u = nn.Parameter(_l2normalize(w.data.new_empty(height).normal_(0, 1)), requires_grad=False)
        v = nn.Parameter(_l2normalize(w.data.new_empty(width).normal_(0, 1)), requires_grad=False)
        w_bar = nn.Parameter(w.data)
        del module._parameters["weight"]
        module.register_parameter("weight_u", u)
        module.register_parameter("weight_v", v)
        module.register_parameter("weight_bar", w_bar)

    def sigma_step(self):
        """One power step on the device (u, v updated in place); returns the one-element tensor 1 / sigma."""
        m = self.module
        return ops.gan_spectral_sigma(m.weight_bar.detach(), m.weight_u.detach(), m.weight_v.detach(), arch.GAN_SN_EPS)

    def save_for_wgrad(self, saved, tag, inv):
        """What the spectral-norm backward of this forward needs, under `tag`: W_bar and the bias (the parameters themselves, so
        that autograd sees a rewrite), 1 / sigma, and COPIES of the u, v the power step just left — the next forward overwrites
        the module's own through a C call that no version counter sees."""
        m = self.module
        saved[f"w{tag}"], saved[f"b{tag}"], saved[f"inv{tag}"] = m.weight_bar.detach(), m.bias.detach(), inv
        saved[f"u{tag}"], saved[f"v{tag}"] = m.weight_u.detach().clone(), m.weight_v.detach().clone()


class Self_Attn(nn.Module):
    """Parameter container of the self-attention block (GAN_models.py): three spectrally normalised 1x1 convolutions C -> C and
    the scalar gamma (initially 0)."""

    def __init__(self, in_dim):
        super().__init__()
        self.chanel_in = in_dim
        for name in arch.GAN_ATTENTION_CONVS:
            setattr(self, name, SpectralNorm(nn.Conv2d(in_dim, in_dim, kernel_size=1)))
        self.gamma = nn.Parameter(torch.zeros(1))


def attention_core(q, k, v):
    """q, k, v [N, C, P] (views with one unit inner stride) -> (o [N, C, P], a [N, P, P]): a = softmax_j(sum_c q[c][i] k[c][j]),
    o[c][i] = sum_j v[c][j] a[i][j].  Two products on the native GEMM (ops.bgemm) and the row softmax."""
    a = ops.bgemm(q.transpose(1, 2), k)
    ops.gan_softmax_rows(a, out=a)
    return ops.bgemm(v, a.transpose(1, 2)), a


def attention_core_bwd(q, k, v, a, do):
    """[dq; dk; dv] stacked as [N, 3C, P] for do = d loss / d o: four products and the softmax backward."""
    N, C, P = do.shape
    d = torch.empty((N, 3 * C, P), device=do.device, dtype=torch.float32)
    dA = ops.bgemm(do.transpose(1, 2), v)                          # dA[i][j] = sum_c do[c][i] v[c][j]
    ops.bgemm(do, a, out=d[:, 2 * C:])                             # dv[c][j] = sum_i do[c][i] a[i][j]
    ops.gan_softmax_rows_bwd(a, dA, out=dA)
    ops.bgemm(k, dA.transpose(1, 2), out=d[:, :C])                 # dq[c][i] = sum_j dE[i][j] k[c][j]
    ops.bgemm(q, dA, out=d[:, C:2 * C])                            # dk[c][j] = sum_i q[c][i] dE[i][j]
    return d


class _InputGrad(torch.autograd.Function):
    """Discriminator_x64._forward with what the backward needs saved; backward returns d x only (the parameters are frozen)."""

    @staticmethod
    def forward(ctx, x, module):
        saved = {}
        out, f4 = module._forward(x.detach(), saved)
        ctx.module, ctx.in_hw = module, tuple(x.shape[2:])
        ctx.saved_keys = tuple(saved)
        ctx.save_for_backward(*saved.values())
        ctx.set_materialize_grads(False)
        return out, f4

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_f4):
        if g_out is None and g_f4 is None:
            return None, None
        saved = dict(zip(ctx.saved_keys, ctx.saved_tensors))
        return ctx.module._input_grad(saved, g_out, g_f4, ctx.in_hw), None


class _Train(torch.autograd.Function):
    """The same forward with the 21 parameters as inputs (`names`: their state_dict names, in the order of `params`), so that
    autograd accumulates into their .grad; backward fills the parameters that require grad, and d x only if x does."""

    @staticmethod
    def forward(ctx, x, module, names, *params):
        saved = {}
        out, f4 = module._forward(x.detach(), saved, train=True)
        ctx.module, ctx.in_hw, ctx.names = module, tuple(x.shape[2:]), names
        ctx.saved_keys = tuple(saved)
        ctx.save_for_backward(*saved.values())
        ctx.set_materialize_grads(False)
        return out, f4

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_f4):
        if g_out is None and g_f4 is None:
            return (None,) * (3 + len(ctx.names))
        saved = dict(zip(ctx.saved_keys, ctx.saved_tensors))
        need = {n for n, hot in zip(ctx.names, ctx.needs_input_grad[3:]) if hot}
        dx, grads = ctx.module._backward(saved, g_out, g_f4, ctx.in_hw, ctx.needs_input_grad[0], need)
        return (dx, None, None) + tuple(grads.get(n) for n in ctx.names)


class Discriminator_x64(nn.Module):
    """Input [N, in_size, H, W] (train.py: the Lab frame next to its predecessor, 6 channels), H x W at least 192 x 384.
    forward(x) -> (output [N, 1], feature4 = layer4's activation)."""

    def __init__(self, in_size=6, ndf=64):
        super().__init__()
        self.in_size, self.ndf = in_size, ndf
        for name, cin, cout in arch.gan_conv_plan(in_size, ndf):
            setattr(self, name, nn.Sequential(SpectralNorm(nn.Conv2d(cin, cout, 4, 2, 1)), nn.LeakyReLU(SLOPE)))
            if name == arch.GAN_ATTENTION_AFTER:
                self.attention = Self_Attn(cout)
        self.last = SpectralNorm(nn.Conv2d(ndf * arch.GAN_CH_MULT[-1], 1, list(arch.GAN_LAST_KSIZE), 1, 0))

    # -- the opt-in to the parameter gradients
    @property
    def parameter_training(self):
        """Whether backward also gives the module's own 21 parameter gradients (set_parameter_training)."""
        return self.__dict__.get("_parameter_training", False)

    def set_parameter_training(self, flag=True):
        """Opt in to (or out of) the parameter gradients: with it on, under grad mode, a parameter or an input requiring grad sends
        forward through the training path, whose backward fills every parameter that requires grad (and the input gradient if the
        input requires grad); with it off (the default) an unfrozen parameter under grad mode is refused.  Not part of
        state_dict(); kept by pickling / copy.deepcopy.  Returns self."""
        self.__dict__["_parameter_training"] = bool(flag)
        return self

    def _trainable_named_parameters(self):
        """The 21: W_bar and bias of the ten SpectralNorm modules and gamma (weight_u / weight_v are state, not parameters to train)."""
        return [(n, p) for n, p in self.named_parameters() if not n.endswith(("weight_u", "weight_v"))]

    # -- checks
    def _check(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.in_size:
            raise RuntimeError(f"Discriminator_x64: input must be a tensor [N, {self.in_size}, H, W] (got "
                               f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)})")
        H, W = x.shape[2:]
        h6, w6 = arch.gan_out_hw(H, W)
        if h6 < arch.GAN_LAST_KSIZE[0] or w6 < arch.GAN_LAST_KSIZE[1]:
            raise RuntimeError(f"Discriminator_x64: a {H} x {W} input leaves a {h6} x {w6} map after six stride-2 layers, smaller "
                               f"than the {arch.GAN_LAST_KSIZE[0]} x {arch.GAN_LAST_KSIZE[1]} filter of `last`; the smallest "
                               "input is 192 x 384")
        if torch.is_grad_enabled() and not self.parameter_training:
            hot = [n for n, p in self.named_parameters() if p.requires_grad]
            if hot:
                raise NotImplementedError(
                    f"Discriminator_x64: parameter {hot[0]} (and {len(hot) - 1} more) requires grad while autograd is recording, "
                    "but the discriminator's parameter gradients are not built yet into this graph: by default the module is a "
                    "frozen critic (forward and input gradient). Call discriminator.set_parameter_training() to opt in to its "
                    "own parameter gradients (train.py's discriminator step); or call discriminator.requires_grad_(False) "
                    "around the generator's step, or run it under torch.no_grad().")
        if not x.is_cuda:
            raise RuntimeError(f"Discriminator_x64: input is on {x.device}; the MI355X HIP path has no CPU fallback (move the "
                               "module and its inputs to the GPU with .cuda())")

    def forward(self, x):
        self._check(x)
        x = x.float()
        if torch.is_grad_enabled():
            if self.parameter_training:
                named = self._trainable_named_parameters()
                if x.requires_grad or any(p.requires_grad for _, p in named):
                    return _Train.apply(x, self, tuple(n for n, _ in named), *(p for _, p in named))
            elif x.requires_grad:
                return _InputGrad.apply(x, self)
        return self._forward(x.detach())

    # -- the layer walk
    def _sn_layers(self):
        return [getattr(self, name)[0] for name in arch.GAN_LAYERS]

    def _attention_forward(self, x, saved, train=False):
        """y = gamma * (v softmax(q^T k)^T) + x on [N, C, h, w]: three sigma steps, the scaled filters of the three projections
        stacked (one 1x1 launch gives q, k, v), two products on the native GEMM, the row softmax, the residual."""
        att = self.attention
        N, C, h, w = x.shape
        P = h * w
        sns = [getattr(att, name) for name in arch.GAN_ATTENTION_CONVS]
        w_fwd = torch.empty((C, 3 * C), device=x.device, dtype=torch.float32)      # [cin][stacked cout]: dvc_conv2d's ksize-1 pack
        w_bwd = torch.empty((3 * C, C), device=x.device, dtype=torch.float32)      # [stacked cout][cin]: the input gradient's pack
        for i, (name, sn) in enumerate(zip(arch.GAN_ATTENTION_CONVS, sns)):
            inv = sn.sigma_step()
            ops.gan_sn_weight(sn.module.weight_bar.detach(), inv, scaled=w_bwd[i * C:(i + 1) * C], scaled_t=w_fwd, col=i * C)
            if train:
                sn.save_for_wgrad(saved, "_" + name, inv)
        bias = torch.cat([sn.module.bias.detach() for sn in sns])
        qkv = ops.conv2d(x, w_fwd.view(C, 1, 3 * C), bias, ksize=1, pad=0, tune=False).view(N, 3 * C, P)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        o, a = attention_core(q, k, v)
        y = ops.gan_scale_add(o.view(N, C, h, w), att.gamma.detach(), x)
        if saved is not None:
            saved.update(qkv=qkv, att=a, w_att=w_bwd, gamma=att.gamma.detach())
            if train:
                saved["y_att"] = y              # layer5's input (o is recomputed from qkv and att in the backward, not kept)
        return y

    def _attention_backward(self, saved, dy, need=(), grads=None, want_dx=True):
        """d loss / d x of the attention block for dy = d loss / d y (None with want_dx off); the gradients of gamma and of the
        three projections named in `need` go into `grads`."""
        qkv, a, w_bwd = saved["qkv"], saved["att"], saved["w_att"]
        N, C, h, w = dy.shape
        P = h * w
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        if "attention.gamma" in need:
            grads["attention.gamma"] = ops.gan_dot(dy, ops.bgemm(v, a.transpose(1, 2)))     # o, as the forward made it
        hot = [name for name in arch.GAN_ATTENTION_CONVS if self._sn_hot(f"attention.{name}.module", need)]
        if not (want_dx or hot):
            return None
        do = ops.gan_scale_add(dy, saved["gamma"]).view(N, C, P)
        d = attention_core_bwd(q, k, v, a, do)                     # [dq; dk; dv]
        if hot:
            # the three plain weight gradients as one 1x1 weight gradient over the stacked channels, then sigma per projection
            G, db = ops.warp_k1_wgrad(d, saved["a4"].view(N, C, P))
            for i, name in enumerate(arch.GAN_ATTENTION_CONVS):
                self._sn_grads(f"attention.{name}.module", "_" + name, G[i * C:(i + 1) * C], db[i * C:(i + 1) * C], saved, need, grads)
        if not want_dx:
            return None
        # dx = dy + W_q^T dq + W_k^T dk + W_v^T dv: one 1x1 launch over the stacked channels, dy as its residual
        return ops.conv2d(d.view(N, 3 * C, h, w), w_bwd.view(3 * C, 1, C), None, ksize=1, pad=0, residual=dy, tune=False)

    def _forward(self, x, saved=None, train=False):
        x = x.contiguous()
        a = x
        feature4 = None
        if train:
            saved["x"] = x
        for i, (name, sn) in enumerate(zip(arch.GAN_LAYERS, self._sn_layers()), 1):
            inv = sn.sigma_step()
            a = ops.gan_conv4s2(a, sn.module.weight_bar.detach(), sn.module.bias.detach(), inv, slope=SLOPE)
            if saved is not None:
                saved[f"a{i}"], saved[f"inv{i}"], saved[f"w{i}"] = a, inv, sn.module.weight_bar.detach()
                if train:
                    sn.save_for_wgrad(saved, i, inv)
            if name == arch.GAN_ATTENTION_AFTER:
                feature4 = a
                a = self._attention_forward(a, saved, train)
        inv = self.last.sigma_step()
        out = ops.gan_last(a, self.last.module.weight_bar.detach(), self.last.module.bias.detach(), inv)
        if saved is not None:
            saved["inv_last"], saved["w_last"] = inv, self.last.module.weight_bar.detach()
            if train:
                self.last.save_for_wgrad(saved, "_last", inv)
        return out, feature4

    def _input_grad(self, saved, g_out, g_f4, in_hw):
        """d loss / d x for g_out = d loss / d output [N, 1] and g_f4 = d loss / d feature4 (either may be None): the walk of
        _backward with nothing asked for but the input gradient."""
        return self._backward(saved, g_out, g_f4, in_hw)[0]

    @staticmethod
    def _sn_hot(prefix, need):
        return prefix + ".weight_bar" in need or prefix + ".bias" in need

    @staticmethod
    def _sn_grads(prefix, tag, G, db, saved, need, grads):
        """From the plain weight gradient G and the bias gradient db of a SpectralNorm module: d loss / d W_bar through sigma."""
        if prefix + ".weight_bar" in need:
            grads[prefix + ".weight_bar"] = ops.gan_sn_wgrad(G, saved[f"w{tag}"], saved[f"u{tag}"], saved[f"v{tag}"], saved[f"inv{tag}"])
        if prefix + ".bias" in need:
            grads[prefix + ".bias"] = db.clone()        # (db is a view into G's buffer: do not keep that alive as a .grad)

    def _backward(self, saved, g_out, g_f4, in_hw, need_x=True, need=()):
        """(d loss / d x or None, {name: gradient}) for g_out = d loss / d output [N, 1] and g_f4 = d loss / d feature4 (either may
        be None).  Every dgrad reads a gradient at a pre-activation: the LeakyReLU derivative of layer k is applied where the
        gradient at its output is written (the store end of layer k+1's dgrad, of `last`'s backward, or — behind the attention
        block — dvc_gan_lrelu_bwd); so every weight gradient reads the same tensor as the dgrad next to it.  The walk stops below
        the lowest layer anything is asked of: with need_x off, layer1's dgrad is not launched.  A parameter no seeded output
        depends on gets no entry.
        The filters and gamma are the tensors saved with the graph, like 1 / sigma: a parameter changed in place between forward
        and backward (load_state_dict, an optimiser step) makes autograd refuse the backward instead of mixing old and new."""
        wb = [saved[f"w{i}"] for i in range(1, 7)]
        act = [None] + [saved[f"a{i}"] for i in range(1, 7)]
        inv = [None] + [saved[f"inv{i}"] for i in range(1, 7)]
        grads = {}
        layer = [None] + [f"{name}.0.module" for name in arch.GAN_LAYERS]
        lowest = min((i for i in range(1, 7) if self._sn_hot(layer[i], need)), default=7)
        att_hot = any(n.startswith("attention.") for n in need)

        def wanted(level):
            """Is anything asked of the walk below `level` (6 .. 1: the input side of that layer; 4.5: the attention block)?"""
            return need_x or lowest <= level or (att_hot and level >= 4.5)

        def wgrad(i, dz, x_in):
            if self._sn_hot(layer[i], need):
                G, db = ops.gan_conv4s2_wgrad(dz, x_in)
                self._sn_grads(layer[i], i, G, db, saved, need, grads)

        d4 = None
        if g_out is not None:
            g = g_out.contiguous()
            if self._sn_hot("last.module", need):
                G, db = ops.gan_last_wgrad(g, act[6])
                self._sn_grads("last.module", "_last", G, db, saved, need, grads)
            if wanted(6):
                dz6 = ops.gan_last_bwd(g, saved["w_last"], saved["inv_last"], act[6], slope=SLOPE)
                wgrad(6, dz6, act[5])
                if wanted(5):
                    dz5 = ops.gan_conv4s2_dgrad(dz6, wb[5], inv[6], act[5].shape[2:], mask_act=act[5], slope=SLOPE)
                    wgrad(5, dz5, saved.get("y_att"))
                    if wanted(4.5):
                        dy = ops.gan_conv4s2_dgrad(dz5, wb[4], inv[5], act[4].shape[2:])
                        d4 = self._attention_backward(saved, dy, need, grads, wanted(4))
        if (d4 is None and g_f4 is None) or not wanted(4):
            return None, grads
        dz = ops.gan_lrelu_bwd(d4, None if g_f4 is None else g_f4.contiguous(), act[4], SLOPE)
        for i in (4, 3, 2):
            wgrad(i, dz, act[i - 1])
            if not wanted(i - 1):
                return None, grads
            dz = ops.gan_conv4s2_dgrad(dz, wb[i - 1], inv[i], act[i - 1].shape[2:], mask_act=act[i - 1], slope=SLOPE)
        wgrad(1, dz, saved.get("x"))
        return (ops.gan_conv4s2_dgrad(dz, wb[0], inv[1], in_hw) if need_x else None), grads
