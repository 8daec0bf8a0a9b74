"""Non-local weighted average on the HIP kernels — the third N x N softmax-affinity consumer of the training side.

`NonlocalWeightedAverage` of the reference's models/NonlocalNet.py:86-111 (with `find_local_patch`, :12-17), the
non-local smoothness term of training.  Same constructor and forward signature and defaults:

    x_lab   = F.interpolate(x_lab, scale_factor=scale_factor)      nearest
    feature = F.interpolate(feature, size=(H, W))                  nearest
    U       = find_local_patch(feature, patch_size)                [B, C k k, N]
    A       = softmax(U^T U / alpha, dim=-1)                       [B, N, N]
    out     = (A @ x_ab^T)^T .view(B, 2, H, W)                     x_ab = x_lab[:, 1:3].detach()

all of it one call of dvc_nlwa_fwd (csrc/nonlocal_avg.hip): a prep launch does both resizes (ATen's nearest source
indices, bit for bit) and the zero-bordered feature, the fused launch builds the affinities from shifted windows of it
on the fp32 MFMA with an online softmax, a merge launch combines the partial states.  Nothing N x N is materialised.
The output carries no gradient: x_ab is detached by the reference, and its training caller passes `feature` detached.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib, ops
from .ops import _p, _stream

NL_KC = 32   # csrc/nonlocal_avg.hip: the channel chunk the zero-bordered feature's planes are padded to


def _out_size(n, scale_factor):
    """F.interpolate's output size for a scale factor: the integer part of n * scale_factor (in double)."""
    return int(float(n) * float(scale_factor))


def _src_scale_factor(scale_factor):
    """The source-index scale ATen derives from a given factor: float32(1 / scale_factor), the division in double."""
    return float(torch.tensor(1.0 / float(scale_factor), dtype=torch.float32))


def _src_scale_size(n_in, n_out):
    """The source-index scale ATen derives from a given size: float32(n_in) / n_out, in float32."""
    return float(torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32))


def workspace_layout(B, C, patch_size, H, W):
    """Byte offsets and shapes of the prep launch's outputs inside the workspace (include/dvc_hip.h): the zero-bordered
    resized feature F_pad [B, Cp, H + 2p, W + 2p] and the resized ab [B, 2, H, W]."""
    p = patch_size // 2
    Cp = -(-C // NL_KC) * NL_KC
    fpad_shape = (B, Cp, H + 2 * p, W + 2 * p)
    ab_off = (4 * B * Cp * (H + 2 * p) * (W + 2 * p) + 255) // 256 * 256
    return {"fpad": (0, fpad_shape), "ab": (ab_off, (B, 2, H, W))}


def _check_args(x_lab, feature, patch_size, alpha, scale_factor):
    if not (isinstance(x_lab, torch.Tensor) and isinstance(feature, torch.Tensor)):
        raise TypeError("NonlocalWeightedAverage: x_lab and feature must be tensors")
    if x_lab.dim() != 4 or feature.dim() != 4:
        raise ValueError(f"NonlocalWeightedAverage: x_lab and feature must be 4-D [B, C, H, W] (got {tuple(x_lab.shape)}, "
                         f"{tuple(feature.shape)})")
    if x_lab.shape[1] < 3:
        raise ValueError(f"NonlocalWeightedAverage: x_lab needs the L, a, b channels (got {x_lab.shape[1]} channels)")
    if x_lab.shape[0] != feature.shape[0]:
        raise ValueError(f"NonlocalWeightedAverage: batch sizes differ (x_lab {x_lab.shape[0]}, feature {feature.shape[0]})")
    if int(patch_size) != patch_size or patch_size < 1 or patch_size % 2 == 0:
        raise ValueError(f"NonlocalWeightedAverage: patch_size must be an odd integer >= 1 (got {patch_size}); "
                         "find_local_patch's view needs an odd patch")
    alpha = float(alpha)
    if not (alpha > 0.0 and alpha != float("inf")):
        raise ValueError(f"NonlocalWeightedAverage: alpha must be > 0 and finite (got {alpha})")
    if not (float(scale_factor) > 0.0 and float(scale_factor) != float("inf")):
        raise ValueError(f"NonlocalWeightedAverage: scale_factor must be > 0 and finite (got {scale_factor})")
    if feature.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(
            "NonlocalWeightedAverage: no gradient flows to `feature` (the training caller passes it detached); "
            "pass feature.detach() or call under torch.no_grad()")
    if not (x_lab.is_cuda and feature.is_cuda):
        raise RuntimeError("NonlocalWeightedAverage: inputs must be ROCm device tensors; the MI355X HIP path has no CPU "
                           "fallback")


def nonlocal_weighted_average(x_lab, feature, patch_size=3, alpha=0.1, scale_factor=1, workspace=None):
    """Functional form of NonlocalWeightedAverage.forward; returns float32 [B, 2, H, W] on the inputs' device.
    `workspace` (tests only): a uint8 device tensor to run in instead of the cached one, to read the prep outputs
    back through workspace_layout()."""
    _check_args(x_lab, feature, patch_size, alpha, scale_factor)
    lib = _lib.load()
    x_lab = x_lab.detach().contiguous().float()
    feature = feature.detach().contiguous().float()
    ops._need(x_lab, "x_lab")
    ops._need(feature, "feature")
    B, Cx, Hx, Wx = x_lab.shape
    C, Hf, Wf = feature.shape[1:]
    H, W = _out_size(Hx, scale_factor), _out_size(Wx, scale_factor)
    if H < 1 or W < 1:
        raise ValueError(f"NonlocalWeightedAverage: scale_factor {scale_factor} leaves an empty map from {Hx} x {Wx}")
    sx = _src_scale_factor(scale_factor)
    sfh, sfw = _src_scale_size(Hf, H), _src_scale_size(Wf, W)
    k = int(patch_size)
    out = torch.empty((B, 2, H, W), device=x_lab.device, dtype=torch.float32)
    nbytes = lib.dvc_nlwa_workspace_bytes(B, C, k, H, W)
    if workspace is None:
        workspace = ops._workspace(x_lab.device, nbytes, tag="nlwa")
    elif workspace.numel() < nbytes:
        raise ValueError(f"NonlocalWeightedAverage: workspace of {workspace.numel()} bytes, {nbytes} needed")
    _lib.check(lib.dvc_nlwa_fwd(_p(x_lab), Cx, Hx, Wx, _p(feature), C, Hf, Wf, B, H, W, sx, sx, sfh, sfw, k, float(alpha),
                                _p(out), ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), _stream()),
               "dvc_nlwa_fwd")
    return out


class NonlocalWeightedAverage(nn.Module):
    """models/NonlocalNet.py:86-111 on the fused HIP kernel (see the module docstring)."""

    def __init__(self):
        super().__init__()

    def forward(self, x_lab, feature, patch_size=3, alpha=0.1, scale_factor=1):
        # alpha=0.1 if scale_factor=1   (the reference's comment)
        return nonlocal_weighted_average(x_lab, feature, patch_size, alpha, scale_factor)
