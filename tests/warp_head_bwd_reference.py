"""Float64 (or any dtype: float32 gives the CPU yardstick) restatements of the launches WarpNet's backward through its four
heads adds (csrc/warp_head_bwd.hip, dvc_amd/nets.py WarpNet._heads_backward) — TEST INFRASTRUCTURE.  Each function states what one
launch kind computes; tests/test_warp_heads_host.py checks them against autograd through oracle.dvc_oracle, the GPU tests check
the kernels against them.  `defect=` seeds a known mistake (the host tests assert that it breaks the bound):
  "odd_tail"     the last output row / column of a stride-2 layer on an odd-sized input dropped (Ho = H // 2)
  "no_edge"      the replicated rows' gradient not added onto the edge rows
  "block_index"  the 2x2 block sums taken over the wrong elements (blocks indexed as [h][2][2][w])
The sums whose kernels are exact (block sums, edge rows) are written in the kernels' order, so float32 compares bit for bit."""
import torch
import torch.nn.functional as F

import warp_bwd_reference as R


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def head_wgrad(dz_ringed, x_padded, stride=1, defect=None):
    """dvc_warp_head_wgrad: (dW [Cout,Cin,3,3], db [Cout]) of ReflectionPad2d(1) + Conv2d(3, stride) from the zero-ringed dz
    [N,Cout,Ho+2,Wo+2] and the reflect-padded input [N,Cin,H+2,W+2]: tap (ky, kx) multiplies x_padded[s oy + ky][s ox + kx]."""
    dz = dz_ringed[:, :, 1:-1, 1:-1]
    Ho, Wo = dz.shape[2:]
    if defect == "odd_tail":
        Ho, Wo = (x_padded.shape[2] - 2) // stride, (x_padded.shape[3] - 2) // stride
        dz = dz[:, :, :Ho, :Wo]
    dW = dz.new_zeros(dz.shape[1], x_padded.shape[1], 3, 3)
    for ky in range(3):
        for kx in range(3):
            xs = x_padded[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            dW[:, :, ky, kx] = torch.einsum("noyx,niyx->oi", dz, xs)
    return dW, dz.sum((0, 2, 3))


def dilate_ring(dz_ringed, H, W, defect=None):
    """dvc_warp_dilate_ring: [N,C,H+2,W+2], zero except [1 + 2 oy][1 + 2 ox] = dz[oy][ox]."""
    dz = dz_ringed[:, :, 1:-1, 1:-1]
    Ho, Wo = out_hw(H, W, 2)
    assert tuple(dz.shape[2:]) == (Ho, Wo), (dz.shape, H, W)
    if defect == "odd_tail":
        Ho, Wo = H // 2, W // 2
    out = dz.new_zeros(dz.shape[0], dz.shape[1], H + 2, W + 2)
    out[:, :, 1:2 * Ho:2, 1:2 * Wo:2] = dz[:, :, :Ho, :Wo]
    return out


def up2_bwd(g, defect=None):
    """dvc_warp_up2_bwd: 2x2 block sums, (top pair) + (bottom pair)."""
    if defect == "block_index":
        N, C, H, W = g.shape
        return g.reshape(N, C, H // 2, 2, 2, W // 2).sum((3, 4))
    return (g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2]) + (g[:, :, 1::2, 0::2] + g[:, :, 1::2, 1::2])


def rpad_rows_bwd(g, rpad, defect=None):
    """dvc_warp_rpad_rows_bwd: the adjoint of F.pad(x, (0, 0, rpad, rpad), "replicate"): the rows above added onto row 0 (top
    down), then the rows below onto the last row."""
    h = g.shape[2] - 2 * rpad
    out = g[:, :, rpad:rpad + h].clone()
    if defect != "no_edge":
        for k in range(rpad):
            out[:, :, 0] += g[:, :, k]
        for k in range(rpad):
            out[:, :, h - 1] += g[:, :, h + rpad + k]
    return out


def up2(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3)


def _names(hd):
    pre = hd.name + "."
    return f"{pre}{hd.conv_a}", f"{pre}{hd.conv_b}", f"{pre}{hd.prelu_a}.weight", f"{pre}{hd.prelu_b}.weight"


def head_forward(sd, hd, x):
    """oracle.warp_head for the head `hd` (an arch.WarpHead) with what the backward keeps: dict(x, na, ra, pa, nb, rb, out)."""
    ka, kb, sa, sb = _names(hd)

    def conv_norm(t, key, stride):
        z = F.conv2d(R.reflect_pad(t), sd[key + ".weight"], sd[key + ".bias"], stride=stride)
        mean = z.mean((2, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(z.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
        return (z - mean) * rstd, rstd.reshape(-1)

    na, ra = conv_norm(x, ka, 1)
    pa = F.prelu(na, sd[sa])
    nb, rb = conv_norm(up2(pa) if hd.up_mid else pa, kb, hd.stride_b)
    pb = F.prelu(nb, sd[sb])
    return dict(x=x, na=na, ra=ra, pa=pa, nb=nb, rb=rb, out=up2(pb) if hd.up_out else pb)


def head_bwd(sd, hd, s, g, rpad=0, defect=None):
    """The backward walk of one head from the gradient g at its (row-padded) output, launch by launch as
    WarpNet._heads_backward does it.  Returns {parameter name: gradient}."""
    ka, kb, sa, sb = _names(hd)
    grads = {}
    if rpad:
        g = rpad_rows_bwd(g, rpad, defect=defect)
    if hd.up_out:
        g = up2_bwd(g, defect=defect)
    dz, _, sp = R.norm_prelu_bwd(g, s["nb"], s["rb"], sd[sb])
    grads[sb] = sp.sum().reshape(1)
    xb = up2(s["pa"]) if hd.up_mid else s["pa"]
    grads[kb + ".weight"], grads[kb + ".bias"] = head_wgrad(dz, R.reflect_pad(xb), hd.stride_b, defect=defect)
    if hd.stride_b == 2:
        dz = dilate_ring(dz, xb.shape[2], xb.shape[3], defect=defect)
    g = R.fold(R.padded_input_grad(dz, sd[kb + ".weight"]))
    if hd.up_mid:
        g = up2_bwd(g, defect=defect)
    dz, _, sp = R.norm_prelu_bwd(g, s["na"], s["ra"], sd[sa])
    grads[sa] = sp.sum().reshape(1)
    grads[ka + ".weight"], grads[ka + ".bias"] = head_wgrad(dz, R.reflect_pad(s["x"]), 1)
    return grads
