"""Float64 (or any dtype: `dtype=` gives the float32 CPU yardstick) restatements of the launches of WarpNet's backward behind
the trunk tensor (csrc/warp_bwd.hip, dvc_amd/nets.py WarpNet._trunk_backward) — TEST INFRASTRUCTURE.  Each function states what
one launch kind computes; tests/test_warp_backward_host.py checks them against autograd through oracle.dvc_oracle, the GPU tests
check the kernels against them.  `defect=` seeds a known mistake (the host tests assert that it breaks the bound)."""
import sys

import torch
import torch.nn.functional as F

EPS = sys.float_info.epsilon


def up4_bwd(g):
    """dvc_warp_up4_bwd: 4x4 block sums."""
    N, C, H, W = g.shape
    return g.reshape(N, C, H // 4, 4, W // 4, 4).sum((3, 5))


def cn_bwd(t_raw, g, eps=EPS):
    """dvc_warp_cn_bwd: t_raw, g [B,C,P] -> d t_raw of oracle.corr_project's centre-and-normalise."""
    tc = t_raw - t_raw.mean(-1, keepdim=True)
    r = tc.pow(2).sum(1, keepdim=True).sqrt()
    s = r + eps
    k = torch.where(r > 0, (tc * g).sum(1, keepdim=True) / (r * s * s), torch.zeros_like(r))
    dtc = g / s - tc * k
    return dtc - dtc.mean(-1, keepdim=True)


def k1_wgrad(dT, Fin):
    """dvc_warp_k1_wgrad: (dW [Cout,Cin,1,1], db [Cout]) from dT [N,Cout,P], Fin [N,Cin,P]."""
    dT, Fin = dT.flatten(2), Fin.flatten(2)
    return torch.einsum("nop,nip->oi", dT, Fin)[:, :, None, None], dT.sum((0, 2))


def ring(dz):
    return F.pad(dz, (1, 1, 1, 1))


def norm_prelu_bwd(g, n, rstd, a, skip=None, defect=None):
    """dvc_warp_norm_prelu_bwd: (dz zero-ringed [N,C,H+2,W+2], du, slope partial sums [N*C]).  ATen's prelu backward: the
    gradient passes unscaled where u > 0; the slope collects u * g elsewhere (u == 0 included: it adds 0)."""
    u = n if skip is None else n + skip
    pos = u > 0
    du = torch.where(pos, g, a * g)
    part = torch.where(pos, torch.zeros_like(g), u * g).sum((2, 3)).reshape(-1)
    mean_du = du.mean((2, 3), keepdim=True)
    if defect == "no_mean":
        mean_du = torch.zeros_like(mean_du)
    dz = rstd.reshape(n.shape[0], n.shape[1], 1, 1) * (du - mean_du - n * (du * n).mean((2, 3), keepdim=True))
    return ring(dz), du, part


def reflect_pad(x):
    """dvc_warp_reflect_pad."""
    return F.pad(x, (1, 1, 1, 1), mode="reflect")


def fold(gp, skip=None, defect=None):
    """dvc_warp_fold: the adjoint of ReflectionPad2d(1)."""
    H, W = gp.shape[2] - 2, gp.shape[3] - 2
    dx = gp[:, :, 1:-1, 1:-1].clone()
    if defect != "no_fold":
        rows = gp[:, :, :, 1:-1]
        dx[:, :, 1] += rows[:, :, 0]
        dx[:, :, H - 2] += rows[:, :, H + 1]
        cols = gp[:, :, 1:-1, :]
        dx[:, :, :, 1] += cols[:, :, :, 0]
        dx[:, :, :, W - 2] += cols[:, :, :, W + 1]
        for py, y in ((0, 1), (H + 1, H - 2)):
            for px, x in ((0, 1), (W + 1, W - 2)):
                dx[:, :, y, x] += gp[:, :, py, px]
    return dx if skip is None else dx + skip


def bwd_weight(w):
    """The backward filter transform (nets.vgg_bwd_weight): W^T flipped, [Cin][Cout][3][3]."""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def padded_input_grad(dz_ringed, w):
    """ops.conv3x3(dz_ringed, W^T flipped) with zero pad 1: the gradient at the reflect-PADDED input [N,Cin,H+2,W+2]."""
    return F.conv2d(dz_ringed, bwd_weight(w), padding=1)


def padded_wgrad(dz_ringed, x_padded):
    """ops.cvn_wgrad(dz_ringed, x_padded): (dW, db) of the zero-pad-1 3x3 convolution on the (H+2) x (W+2) maps — with a zero
    ring in dz it is the reflect-padded layer's."""
    co, ci = dz_ringed.shape[1], x_padded.shape[1]
    dW = torch.nn.grad.conv2d_weight(x_padded, (co, ci, 3, 3), dz_ringed, padding=1)
    return dW, dz_ringed.sum((0, 2, 3))


def residual_block_forward(sd, prefix, x):
    """oracle.residual_block with what the backward keeps: dict(x, n1, rstd1, p1, n2, rstd2, out)."""
    a = sd[prefix + ".prelu.weight"]

    def conv_norm(t, k):
        z = F.conv2d(reflect_pad(t), sd[f"{prefix}.conv{k}.weight"], sd[f"{prefix}.conv{k}.bias"])
        mean = z.mean((2, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(z.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
        return (z - mean) * rstd, rstd.reshape(-1)

    n1, rstd1 = conv_norm(x, 1)
    p1 = F.prelu(n1, a)
    n2, rstd2 = conv_norm(p1, 2)
    return dict(x=x, n1=n1, rstd1=rstd1, p1=p1, n2=n2, rstd2=rstd2, out=F.prelu(n2 + x, a))


def residual_block_bwd(sd, prefix, s, g, defect=None):
    """The backward walk of one block from the gradient g at its output, launch by launch as WarpNet._trunk_backward does it.
    Returns (dx, {parameter name: gradient})."""
    a = sd[prefix + ".prelu.weight"]
    grads = {}
    dz2, du2, sp2 = norm_prelu_bwd(g, s["n2"], s["rstd2"], a, skip=s["x"], defect=defect)
    grads[prefix + ".conv2.weight"], grads[prefix + ".conv2.bias"] = padded_wgrad(dz2, reflect_pad(s["p1"]))
    g_p1 = fold(padded_input_grad(dz2, sd[prefix + ".conv2.weight"]), defect=defect)
    dz1, _, sp1 = norm_prelu_bwd(g_p1, s["n1"], s["rstd1"], a, defect=defect)
    grads[prefix + ".conv1.weight"], grads[prefix + ".conv1.bias"] = padded_wgrad(dz1, reflect_pad(s["x"]))
    dx = fold(padded_input_grad(dz1, sd[prefix + ".conv1.weight"]), skip=du2, defect=defect)
    grads[prefix + ".prelu.weight"] = (sp2.sum() if defect == "one_site" else sp2.sum() + sp1.sum()).reshape(1)
    return dx, grads
