"""Local weighted average on the HIP stencil — the local half of the training side's smoothness term.

`WeightedAverage_color` of the reference's models/NonlocalNet.py (with `find_local_patch`, :12-17).  Same constructor and
forward signature and defaults:

    x_lab  = F.interpolate(x_lab, scale_factor=scale_factor)                       nearest
    g      = (uncenter_l(x_lab[:, 0:1]), x_lab[:, 1:2], x_lab[:, 2:3])             uncenter_l: + 50
    D      = sum_ch (find_local_patch(g_ch, k) - g_ch) ** 2                        [B, k k, H, W], zero padding k // 2
    w      = softmax(-D / alpha, dim=1)
    out    = cat(sum(w * find_local_patch(a', k), 1), sum(w * find_local_patch(b', k), 1))     (a', b') = x_lab_predict[:, 1:3]

forward one launch of dvc_lwa_fwd, backward one launch of dvc_lwa_bwd (csrc/local_avg.hip): the planes and their halo are
staged in the LDS, nothing k*k-times unfolded is allocated, and autograd keeps only the two inputs and the output.  The
gradient reaches x_lab_predict's ab channels and, when it requires grad, x_lab.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .nonlocal_avg import _out_size, _src_scale_factor
from .ops import _p, _stream

MAX_PATCH = 7    # csrc/local_avg.hip: LW_MAX_K, the largest halo the LDS tiles are sized for
L_OFFSET = 50.0  # uncenter_l


def _check_args(x_lab, x_lab_predict, patch_size, alpha, scale_factor):
    if not (isinstance(x_lab, torch.Tensor) and isinstance(x_lab_predict, torch.Tensor)):
        raise TypeError("WeightedAverage_color: x_lab and x_lab_predict must be tensors")
    if x_lab.dim() != 4 or x_lab_predict.dim() != 4:
        raise ValueError(f"WeightedAverage_color: x_lab and x_lab_predict must be 4-D [B, C, H, W] (got {tuple(x_lab.shape)}, "
                         f"{tuple(x_lab_predict.shape)})")
    if x_lab.shape[1] < 3 or x_lab_predict.shape[1] < 3:
        raise ValueError(f"WeightedAverage_color: both inputs need the L, a, b channels (got {x_lab.shape[1]} and "
                         f"{x_lab_predict.shape[1]} channels)")
    if x_lab.shape[0] != x_lab_predict.shape[0]:
        raise ValueError(f"WeightedAverage_color: batch sizes differ (x_lab {x_lab.shape[0]}, x_lab_predict "
                         f"{x_lab_predict.shape[0]})")
    if int(patch_size) != patch_size or patch_size < 1 or patch_size % 2 == 0:
        raise ValueError(f"WeightedAverage_color: patch_size must be an odd integer >= 1 (got {patch_size}); "
                         "find_local_patch's view needs an odd patch")
    if patch_size > MAX_PATCH:
        raise NotImplementedError(f"WeightedAverage_color: patch_size {patch_size} is above the HIP stencil's limit of "
                                  f"{MAX_PATCH}")
    alpha = float(alpha)
    if not (alpha > 0.0 and alpha != float("inf")):
        raise ValueError(f"WeightedAverage_color: alpha must be > 0 and finite (got {alpha})")
    if not (float(scale_factor) > 0.0 and float(scale_factor) != float("inf")):
        raise ValueError(f"WeightedAverage_color: scale_factor must be > 0 and finite (got {scale_factor})")
    H, W = _out_size(x_lab.shape[2], scale_factor), _out_size(x_lab.shape[3], scale_factor)
    if (H, W) != tuple(x_lab_predict.shape[2:]):
        raise ValueError(f"WeightedAverage_color: x_lab resized by {scale_factor} is {H} x {W}, x_lab_predict is "
                         f"{x_lab_predict.shape[2]} x {x_lab_predict.shape[3]}")
    if not (x_lab.is_cuda and x_lab_predict.is_cuda):
        raise RuntimeError("WeightedAverage_color: inputs must be ROCm device tensors; the MI355X HIP path has no CPU "
                           "fallback")


class _LocalAverage(torch.autograd.Function):
    """guide [B, 3, Hx, Wx] (L, a, b; nearest-resized by `scale_factor` inside the tile load), values [B, 2, H, W] (a', b'),
    both float32 contiguous -> [B, 2, H, W]."""

    @staticmethod
    def _call_args(guide, values, k, alpha, scale_factor):
        B, _, Hx, Wx = guide.shape
        H, W = values.shape[2:]
        sx = _src_scale_factor(scale_factor)
        return (_p(guide), 3, Hx, Wx, _p(values), 2, 0, B, H, W, sx, sx, L_OFFSET, k, alpha)

    @staticmethod
    def forward(ctx, guide, values, k, alpha, scale_factor):
        ops._need(guide, "x_lab")
        ops._need(values, "x_lab_predict")
        y = torch.empty_like(values)
        _lib.check(_lib.load().dvc_lwa_fwd(*_LocalAverage._call_args(guide, values, k, alpha, scale_factor), _p(y), _stream()),
                   "dvc_lwa_fwd")
        ctx.save_for_backward(guide, values, y)
        ctx.conf = (k, alpha, scale_factor)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        guide, values, y = ctx.saved_tensors
        k, alpha, scale_factor = ctx.conf
        G = G.contiguous()
        ops._need(G, "grad_output")
        dv = torch.empty_like(values)
        # the guide only asks for a gradient at scale 1 (weighted_average_color resizes it in torch otherwise)
        dg = torch.empty_like(guide) if ctx.needs_input_grad[0] else None
        if dg is not None and guide.shape[2:] != values.shape[2:]:
            raise RuntimeError("WeightedAverage_color: the guide's gradient is only defined at scale_factor 1")
        _lib.check(_lib.load().dvc_lwa_bwd(*_LocalAverage._call_args(guide, values, k, alpha, scale_factor), _p(G), _p(y),
                                           _p(dv), _p(dg), _stream()), "dvc_lwa_bwd")
        return dg, dv, None, None, None


def weighted_average_color(x_lab, x_lab_predict, patch_size=3, alpha=1, scale_factor=1):
    """Functional form of WeightedAverage_color.forward; returns float32 [B, 2, H, W] on the inputs' device."""
    _check_args(x_lab, x_lab_predict, patch_size, alpha, scale_factor)
    # the channel slices, casts and copies are torch's: so are their adjoints and the zero gradients of the unused channels
    guide = x_lab[:, 0:3]
    if guide.requires_grad and torch.is_grad_enabled() and float(scale_factor) != 1.0:
        guide = F.interpolate(guide, scale_factor=scale_factor)    # torch's resize carries the gradient back
        scale_factor = 1
    guide = guide.float().contiguous()
    values = x_lab_predict[:, 1:3].float().contiguous()
    return _LocalAverage.apply(guide, values, int(patch_size), float(alpha), scale_factor)


class WeightedAverage_color(nn.Module):
    """models/NonlocalNet.py's WeightedAverage_color on the fused HIP stencil (see the module docstring)."""

    def __init__(self):
        super().__init__()

    def forward(self, x_lab, x_lab_predict, patch_size=3, alpha=1, scale_factor=1):
        return weighted_average_color(x_lab, x_lab_predict, patch_size, alpha, scale_factor)
