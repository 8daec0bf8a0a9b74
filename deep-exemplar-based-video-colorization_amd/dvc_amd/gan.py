"""Discriminator_x64 (models/GAN_models.py:104-157, models/spectral_normalization.py) as a frozen critic on the kernels of
csrc/gan.hip: the forward and the gradient back to the input — what the generator's adversarial term needs (train.py builds
`discriminator(torch.cat(...))` on the generated frames and back-propagates into the generator).

    from dvc_amd.gan import Discriminator_x64        # instead of `from models.GAN_models import Discriminator_x64`

Same constructor, the same state_dict keys and the same `(output, feature4)` return value as the reference; every forward runs
one power step per SpectralNorm module and updates weight_u / weight_v in place, in train() and in eval(), as the reference
does.  The discriminator's own parameter gradients (the gradient through sigma among them) are NOT built: with grad mode on, a
parameter that requires grad is refused — freeze the module (`requires_grad_(False)`) around the generator's step.

Gradient contract, as for WarpNet's heads: with every parameter frozen, grad mode on and an input that requires grad, both outputs
are differentiable and their backward fills the input gradient only; the values are bit-identical to the no-grad forward from the
same u / v state.  Launch sequence and where the LeakyReLU masks sit: DESIGN.md, "Discriminator_x64".
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
        if torch.is_grad_enabled():
            hot = [n for n, p in self.named_parameters() if p.requires_grad]
            if hot:
                raise NotImplementedError(
                    f"Discriminator_x64: parameter {hot[0]} (and {len(hot) - 1} more) requires grad while autograd is recording, "
                    "but the discriminator's parameter gradients are not built yet: this module is a frozen critic (forward and "
                    "input gradient). Call discriminator.requires_grad_(False) around the generator's step, or run it under "
                    "torch.no_grad().")
        if not x.is_cuda:
            raise RuntimeError(f"Discriminator_x64: input is on {x.device}; the MI355X HIP path has no CPU fallback (move the "
                               "module and its inputs to the GPU with .cuda())")

    def forward(self, x):
        self._check(x)
        x = x.float()
        if torch.is_grad_enabled() and x.requires_grad:
            return _InputGrad.apply(x, self)
        return self._forward(x.detach())

    # -- the layer walk
    def _sn_layers(self):
        return [getattr(self, name)[0] for name in arch.GAN_LAYERS]

    def _attention_forward(self, x, saved):
        """y = gamma * (v softmax(q^T k)^T) + x on [N, C, h, w]: three sigma steps, the scaled filters of the three projections
        stacked (one 1x1 launch gives q, k, v), two products on the native GEMM, the row softmax, the residual."""
        att = self.attention
        N, C, h, w = x.shape
        P = h * w
        sns = [getattr(att, name) for name in arch.GAN_ATTENTION_CONVS]
        w_fwd = torch.empty((C, 3 * C), device=x.device, dtype=torch.float32)      # [cin][stacked cout]: dvc_conv2d's ksize-1 pack
        w_bwd = torch.empty((3 * C, C), device=x.device, dtype=torch.float32)      # [stacked cout][cin]: the input gradient's pack
        for i, sn in enumerate(sns):
            ops.gan_sn_weight(sn.module.weight_bar.detach(), sn.sigma_step(), scaled=w_bwd[i * C:(i + 1) * C], scaled_t=w_fwd,
                              col=i * C)
        bias = torch.cat([sn.module.bias.detach() for sn in sns])
        qkv = ops.conv2d(x, w_fwd.view(C, 1, 3 * C), bias, ksize=1, pad=0, tune=False).view(N, 3 * C, P)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        o, a = attention_core(q, k, v)
        y = ops.gan_scale_add(o.view(N, C, h, w), att.gamma.detach(), x)
        if saved is not None:
            saved.update(qkv=qkv, att=a, w_att=w_bwd, gamma=att.gamma.detach())
        return y

    def _attention_backward(self, saved, dy):
        """d loss / d x of the attention block for dy = d loss / d y."""
        qkv, a, w_bwd = saved["qkv"], saved["att"], saved["w_att"]
        N, C, h, w = dy.shape
        P = h * w
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        do = ops.gan_scale_add(dy, saved["gamma"]).view(N, C, P)
        d = attention_core_bwd(q, k, v, a, do)                     # [dq; dk; dv]
        # dx = dy + W_q^T dq + W_k^T dk + W_v^T dv: one 1x1 launch over the stacked channels, dy as its residual
        return ops.conv2d(d.view(N, 3 * C, h, w), w_bwd.view(3 * C, 1, C), None, ksize=1, pad=0, residual=dy, tune=False)

    def _forward(self, x, saved=None):
        x = x.contiguous()
        a = x
        feature4 = None
        for i, (name, sn) in enumerate(zip(arch.GAN_LAYERS, self._sn_layers()), 1):
            inv = sn.sigma_step()
            a = ops.gan_conv4s2(a, sn.module.weight_bar.detach(), sn.module.bias.detach(), inv, slope=SLOPE)
            if saved is not None:
                saved[f"a{i}"], saved[f"inv{i}"], saved[f"w{i}"] = a, inv, sn.module.weight_bar.detach()
            if name == arch.GAN_ATTENTION_AFTER:
                feature4 = a
                a = self._attention_forward(a, saved)
        inv = self.last.sigma_step()
        out = ops.gan_last(a, self.last.module.weight_bar.detach(), self.last.module.bias.detach(), inv)
        if saved is not None:
            saved["inv_last"], saved["w_last"] = inv, self.last.module.weight_bar.detach()
        return out, feature4

    def _input_grad(self, saved, g_out, g_f4, in_hw):
        """d loss / d x for g_out = d loss / d output [N, 1] and g_f4 = d loss / d feature4 (either may be None).  Every dgrad reads
        a gradient at a pre-activation: the LeakyReLU derivative of layer k is applied where the gradient at its output is
        written (the store end of layer k+1's dgrad, of `last`'s backward, or — behind the attention block — dvc_gan_lrelu_bwd).
        The filters and gamma are the tensors saved with the graph, like 1 / sigma: a parameter changed in place between forward
        and backward (load_state_dict, an optimiser step) makes autograd refuse the backward instead of mixing old and new."""
        wb = [saved[f"w{i}"] for i in range(1, 7)]
        act = [None] + [saved[f"a{i}"] for i in range(1, 7)]
        inv = [None] + [saved[f"inv{i}"] for i in range(1, 7)]
        d4 = None
        if g_out is not None:
            dz6 = ops.gan_last_bwd(g_out.contiguous(), saved["w_last"], saved["inv_last"], act[6], slope=SLOPE)
            dz5 = ops.gan_conv4s2_dgrad(dz6, wb[5], inv[6], act[5].shape[2:], mask_act=act[5], slope=SLOPE)
            dy = ops.gan_conv4s2_dgrad(dz5, wb[4], inv[5], act[4].shape[2:])
            d4 = self._attention_backward(saved, dy)
        dz = ops.gan_lrelu_bwd(d4, None if g_f4 is None else g_f4.contiguous(), act[4], SLOPE)
        for i in (4, 3, 2):
            dz = ops.gan_conv4s2_dgrad(dz, wb[i - 1], inv[i], act[i - 1].shape[2:], mask_act=act[i - 1], slope=SLOPE)
        return ops.gan_conv4s2_dgrad(dz, wb[0], inv[1], in_hw)
