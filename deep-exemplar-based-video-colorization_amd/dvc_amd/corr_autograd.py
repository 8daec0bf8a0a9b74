"""Differentiable fused correlation — the training-side reuse of the north-star kernel.

The reference trains through `WarpNet.forward` (train.py:402-427 calls frame_colorization under autograd; models/
NonlocalNet.py:477-500): f = theta^T phi, softmax(f / T) with T = 0.01, y = p . B_lab, similarity = max_j f.  Here the
forward is the fused HIP kernel (dvc_corr_fwd) and the backward recomputes the affinities block by block instead of
keeping the P x P matrices autograd would have saved (4 x 107 MB per image at 216x384):

    for each block of R query rows:
        F      = theta_blk^T phi                                   batched GEMM             [R, P]
        dS     = p (g.B_j - g.y_i) / T  (+ d sim at the arg-max)   dvc_corr_softmax_bwd     [R, P] (or [P, R] too)
        d phi += theta_blk dS ;  d theta_blk = phi dS^T            batched GEMMs

The three products are plain fp32 GEMMs, issued by dvc_amd.block_products: the vendor's batched GEMM by default (ops.bmm), this
library's 1x1-convolution engine with per-image filters under DVC_GEMM_LIB=0, this library's own strided fp32 GEMM (ops.bgemm)
under block_products.set_backend("native").

Gradients flow to theta and phi (the centred, normalised projections); the pooled exemplar colours are data (no
gradient).  r05: the WTA re-weighting (`WTA_scale_weight != 1`, NonlocalNet.py:288-327; dead in both reference drivers) is
differentiated too, with the reference's own backward rule — factor 1 at the row maximum and the CONSTANT 1e-4 elsewhere,
whatever the scale (NonlocalNet.py:322) — and the similarity map's gradient untouched (it is taken before the re-weighting,
NonlocalNet.py:481-483).  Parity against autograd through the oracle's `correlate`: tests/test_gpu_corr_backward.py.
"""
import torch

from . import _lib, ops
from .block_products import block_products
from .ops import _p, _stream

ROW_BLOCK = 2048
BLOCK_BYTES = 768 << 20     # cap of one [images, R, P] fp32 buffer of the backward pass (three of them live at a time)


class _FusedCorrelation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, phi, blab, temperature, h, w, wta_scale=1.0):
        theta, phi, blab = theta.contiguous(), phi.contiguous(), blab.contiguous()
        res = ops.corr_fwd(theta.detach(), phi.detach(), blab.detach(), float(temperature), h, w, wta_scale=float(wta_scale),
                           want_small=True, want_argmax=True, want_up=False)
        y, sim, amax = res["y_small"], res["sim_small"], res["argmax"]
        ctx.save_for_backward(theta.detach(), phi.detach(), blab.detach(), y, sim, amax)
        ctx.temperature, ctx.hw, ctx.wta = float(temperature), (h, w), float(wta_scale)
        ctx.mark_non_differentiable(amax)
        return y, sim, amax

    @staticmethod
    def backward(ctx, gy, gsim, _gamax):
        """The whole batch per launch: the three recompute products are batched (block_products) and dvc_corr_softmax_bwd takes
        the batch as a grid dimension.  Images are processed `chunk` at a time so that the three [chunk, R, P] fp32 buffers stay
        within BLOCK_BYTES."""
        theta, phi, blab, y, sim, amax = ctx.saved_tensors
        h, w = ctx.hw
        B, C, P = theta.shape
        lib = _lib.load()
        need_sim = gsim is not None and bool((gsim != 0).any())
        gy = torch.zeros_like(y) if gy is None else gy.contiguous().float()
        gsim_c = gsim.contiguous().float().view(B, P) if need_sim else None
        d_theta = torch.zeros_like(theta)
        d_phi = torch.zeros_like(phi)
        R = min(ROW_BLOCK, (P + 63) // 64 * 64)
        prod = block_products(theta, phi, (h, w), R, max(1, min(B, BLOCK_BYTES // (4 * R * P))), want_rows=True, want_cols=True)
        chunk = prod.chunk
        lsum = torch.empty(chunk * 3 * R, device=theta.device, dtype=torch.float32)   # row maxima, row sums, raw row maxima of a block
        yv, gyv, blv, amv, simv = y.view(B, 3, P), gy.view(B, 3, P), blab.view(B, 3, P), amax.view(B, P), sim.view(B, P)
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            sl_b = slice(b0, b0 + nb)
            prod.images(sl_b)
            for i0 in range(0, P, R):
                rows = min(R, P - i0)
                F, ld = prod.scores(i0, rows)                    # F[b, i, :] = sum_c theta[b, c, i0 + i] phi[b, c, :]
                dS, dST = prod.ds_targets()
                # (the per-row operands start at row i0 of each image: views whose first element is that row's)
                rc = lib.dvc_corr_softmax_bwd(
                    _p(F), _p(blv[sl_b]), _p(gyv[sl_b, :, i0:]), _p(yv[sl_b, :, i0:]), _p(simv[sl_b, i0:]),
                    _p(gsim_c[sl_b, i0:]) if need_sim else None, _p(amv[sl_b, i0:]) if need_sim else None,
                    ctx.temperature, ctx.wta, nb, rows, P, P, ld, _p(lsum), _p(dS), _p(dST), _stream())
                _lib.check(rc, "dvc_corr_softmax_bwd")
                prod.grad_cols_accumulate(d_phi)                 # d phi[b, c, j] += sum_i theta[b, c, i0 + i] dS[b, i, j]
                prod.grad_rows(d_theta)                          # d theta[b, c, i0 + i] = sum_j phi[b, c, j] dS[b, i, j]
        return d_theta, d_phi, None, None, None, None, None


def fused_correlation(theta, phi, B_lab_pooled, temperature, h, w, WTA_scale_weight=1):
    """theta, phi: [B, 256, P] centred + L2-normalised projections (what `WarpNet.project` / ops.corr_prepare produce),
    B_lab_pooled: [B, 3, P] = avg_pool2d(B_lab_map, 4) flattened, P = h * w.
    Returns (y [B, 3, h, w], similarity [B, 1, h, w], argmax [B, P]) like the low-resolution stage of WarpNet.forward
    (NonlocalNet.py:477-499 before the x4 nearest upsampling); differentiable w.r.t. theta and phi.
    `WTA_scale_weight` as in WarpNet.forward (NonlocalNet.py:440,486)."""
    return _FusedCorrelation.apply(theta, phi, B_lab_pooled, temperature, h, w, float(WTA_scale_weight))
