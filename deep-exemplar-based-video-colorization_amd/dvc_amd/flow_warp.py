"""Flow warp on the HIP kernels — the warp of the training side's temporal-consistency term.

`WarpingLayer` of the reference's utils/warping.py, same forward signature:

    get_grid(x):  h = linspace(-1, 1, W) over x,  v = linspace(-1, 1, H) over y                      -> [B, 2, H, W]
    forward(x, flow):
        f[:, 0] = flow[:, 0] / ((W - 1) / 2);  f[:, 1] = flow[:, 1] / ((H - 1) / 2)
        return F.grid_sample(x, (get_grid(x) + f).permute(0, 2, 3, 1))                               bilinear, zeros padding

x [B, C, H, W], flow [B, 2, H, W] (channel 0 the x displacement, channel 1 the y displacement, pixels).  `align_corners`:
False (and None, the constructor's default) is what the unmodified file computes under a torch whose F.grid_sample defaults to
align_corners=False: the sample position is (x + u) W / (W - 1) - 0.5.  True is the exact pixel displacement x + u the file
was written for (torch <= 1.2).  A NaN / inf flow gives NaN in every channel of that output pixel, as torch does; such a pixel
adds nothing to the gradient of x and its flow gradient is NaN.

forward one launch of dvc_flow_warp_fwd; backward dvc_flow_warp_bwd (csrc/flow_warp.hip): the gradient of x is a scatter
summed in exact integer arithmetic — bitwise reproducible and independent of the batch around an image — the gradient of
flow a gather in the same pass.  Autograd keeps only the two inputs; only the gradients that are needed are computed.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .ops import _p, _stream

MAX_HW = 1 << 22   # csrc/flow_warp.hip: FW_MAX_HW, the bound that keeps the integer accumulator from overflowing


def _check_args(x, flow):
    if not (isinstance(x, torch.Tensor) and isinstance(flow, torch.Tensor)):
        raise TypeError("WarpingLayer: x and flow must be tensors")
    if x.dim() != 4 or flow.dim() != 4:
        raise ValueError(f"WarpingLayer: x and flow must be 4-D [B, C, H, W] and [B, 2, H, W] (got {tuple(x.shape)}, "
                         f"{tuple(flow.shape)})")
    if flow.shape[1] != 2:
        raise ValueError(f"WarpingLayer: flow needs 2 channels (x and y displacement; got {flow.shape[1]})")
    if x.shape[0] != flow.shape[0]:
        raise ValueError(f"WarpingLayer: batch sizes differ (x {x.shape[0]}, flow {flow.shape[0]})")
    if tuple(x.shape[2:]) != tuple(flow.shape[2:]):
        raise ValueError(f"WarpingLayer: x is {x.shape[2]} x {x.shape[3]}, flow is {flow.shape[2]} x {flow.shape[3]}")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"WarpingLayer: empty batch or no channels (got {tuple(x.shape)})")
    if x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError(f"WarpingLayer: H and W must be at least 2 (got {x.shape[2]} x {x.shape[3]}): the grid divides by "
                         "(W - 1) / 2")
    if x.shape[2] * x.shape[3] > MAX_HW:
        raise ValueError(f"WarpingLayer: H * W is above 2^22 (got {x.shape[2]} x {x.shape[3]})")
    if not (x.is_cuda and flow.is_cuda):
        raise RuntimeError("WarpingLayer: inputs must be ROCm device tensors; the MI355X HIP path has no CPU fallback")


class _FlowWarp(torch.autograd.Function):
    """x [B, C, H, W], flow [B, 2, H, W], both float32 contiguous -> [B, C, H, W]."""

    @staticmethod
    def forward(ctx, x, flow, align_corners):
        ops._need(x, "x")
        ops._need(flow, "flow")
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        _lib.check(_lib.load().dvc_flow_warp_fwd(_p(x), _p(flow), B, C, H, W, align_corners, _p(y), _stream()),
                   "dvc_flow_warp_fwd")
        ctx.save_for_backward(x, flow)
        ctx.align_corners = align_corners
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        x, flow = ctx.saved_tensors
        want_dx, want_df = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_dx or want_df):
            return None, None, None
        G = G.contiguous()
        ops._need(G, "grad_output")
        B, C, H, W = x.shape
        lib = _lib.load()
        dx = torch.empty_like(x) if want_dx else None
        df = torch.empty_like(flow) if want_df else None
        ws, ws_bytes = None, 0
        if want_dx:
            ws_bytes = lib.dvc_flow_warp_bwd_workspace_bytes(B, C, H, W)
            ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=x.device)   # zeroed by the call, on the stream
        _lib.check(lib.dvc_flow_warp_bwd(_p(x), _p(flow), _p(G), B, C, H, W, ctx.align_corners, _p(dx), _p(df), _p(ws), ws_bytes,
                                         _stream()), "dvc_flow_warp_bwd")
        return dx, df, None


def flow_warp(x, flow, align_corners=False):
    """Functional form of WarpingLayer.forward; returns float32 [B, C, H, W] on the inputs' device."""
    _check_args(x, flow)
    # the casts and copies are torch's: so are their adjoints
    return _FlowWarp.apply(x.float().contiguous(), flow.float().contiguous(), 1 if align_corners else 0)


class WarpingLayer(nn.Module):
    """utils/warping.py's WarpingLayer on the HIP kernels (see the module docstring).  align_corners None or False: today's
    F.grid_sample default; True: exact pixel displacement."""

    def __init__(self, align_corners=None):
        super().__init__()
        self.align_corners = bool(align_corners)

    def forward(self, x, flow):
        return flow_warp(x, flow, self.align_corners)
