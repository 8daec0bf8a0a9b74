"""Test infrastructure: the float64 restatement of NonlocalWeightedAverage (reference models/NonlocalNet.py:86-111, with
`find_local_patch` at :12-17), on the CPU.  Product code under dvc_amd/ and models/ never imports it.

    def find_local_patch(x, patch_size):                                            # NonlocalNet.py:12-17
        N, C, H, W = x.shape
        x_unfold = F.unfold(x, kernel_size=(patch_size, patch_size), padding=(patch_size // 2, patch_size // 2), stride=(1, 1))
        return x_unfold.view(N, x_unfold.shape[1], H, W)

    class NonlocalWeightedAverage(nn.Module):                                       # NonlocalNet.py:86-111
        def forward(self, x_lab, feature, patch_size=3, alpha=0.1, scale_factor=1):
            x_lab = F.interpolate(x_lab, scale_factor=scale_factor)
            batch_size, channel, height, width = x_lab.shape
            feature = F.interpolate(feature, size=(height, width))
            batch_size = x_lab.shape[0]
            x_ab = x_lab[:, 1:3, :, :].detach()
            local_feature = find_local_patch(feature, patch_size)
            local_feature = local_feature.view(batch_size, local_feature.shape[1], -1)
            correlation_matrix = torch.matmul(local_feature.permute(0, 2, 1), local_feature)
            correlation_matrix = nn.functional.softmax(correlation_matrix / alpha, dim=-1)
            weighted_ab = torch.matmul(correlation_matrix, x_ab.view(batch_size, 2, -1).permute(0, 2, 1))
            weighted_ab = weighted_ab.permute(0, 2, 1).contiguous()
            weighted_ab = weighted_ab.view(batch_size, 2, height, width)
            return weighted_ab

The two nearest resizes select values (no arithmetic), so they run in float32 and the rest in `dtype`.
"""
import torch
import torch.nn.functional as F


def resize(x_lab, feature, scale_factor=1):
    """The two interpolations of forward(): (x_lab resized, feature resized to its H x W)."""
    x_lab = F.interpolate(x_lab, scale_factor=scale_factor)
    feature = F.interpolate(feature, size=tuple(x_lab.shape[2:]))
    return x_lab, feature


def find_local_patch(x, patch_size):
    N, C, H, W = x.shape
    x_unfold = F.unfold(x, kernel_size=(patch_size, patch_size), padding=(patch_size // 2, patch_size // 2), stride=(1, 1))
    return x_unfold.view(N, x_unfold.shape[1], H, W)


def nonlocal_weighted_average(x_lab, feature, patch_size=3, alpha=0.1, scale_factor=1, dtype=torch.float64):
    """The reference's forward on CPU tensors, the arithmetic in `dtype` (float64: the restatement; float32: the same
    composition at the precision the reference itself runs in, for the error yardstick)."""
    x_lab, feature = resize(x_lab.detach().cpu().float(), feature.detach().cpu().float(), scale_factor)
    B, _, H, W = x_lab.shape
    x_ab = x_lab[:, 1:3].to(dtype)
    U = find_local_patch(feature.to(dtype), patch_size).view(B, -1, H * W)
    A = torch.softmax(torch.matmul(U.permute(0, 2, 1), U) / alpha, dim=-1)
    out = torch.matmul(A, x_ab.reshape(B, 2, -1).permute(0, 2, 1))
    return out.permute(0, 2, 1).contiguous().view(B, 2, H, W)
