"""Test infrastructure: the restatement of WeightedAverage_color (reference models/NonlocalNet.py, with `find_local_patch`
at :12-17 and `uncenter_l` of utils/util.py:63-64), on the CPU.  Product code under dvc_amd/ and models/ never imports it.

    def forward(self, x_lab, x_lab_predict, patch_size=3, alpha=1, scale_factor=1):
        x_lab = F.interpolate(x_lab, scale_factor=scale_factor)            # nearest
        l = uncenter_l(x_lab[:, 0:1]); a = x_lab[:, 1:2]; b = x_lab[:, 2:3]   # uncenter_l: + 50
        a_predict = x_lab_predict[:, 1:2]; b_predict = x_lab_predict[:, 2:3]
        local_l, local_a, local_b = (find_local_patch(t, patch_size) for t in (l, a, b))
        local_a_predict = find_local_patch(a_predict, patch_size)
        local_b_predict = find_local_patch(b_predict, patch_size)
        local_color_difference = (local_l - l) ** 2 + (local_a - a) ** 2 + (local_b - b) ** 2
        correlation = softmax(-1 * local_color_difference / alpha, dim=1)
        return cat((sum(correlation * local_a_predict, dim=1, keepdim=True),
                    sum(correlation * local_b_predict, dim=1, keepdim=True)), 1)

The nearest resize selects values (no arithmetic), so it runs in float32 and the rest in `dtype`: float64 is the restatement,
float32 the same composition at the precision the reference itself runs in — the error yardstick.
"""
import torch
import torch.nn.functional as F

L_OFFSET = 50.0   # uncenter_l


def find_local_patch(x, patch_size):
    N, C, H, W = x.shape
    x_unfold = F.unfold(x, kernel_size=(patch_size, patch_size), padding=(patch_size // 2, patch_size // 2), stride=(1, 1))
    return x_unfold.view(N, x_unfold.shape[1], H, W)


def compose(x_lab, x_lab_predict, patch_size=3, alpha=1):
    """The body of forward() after the resize, op for op, on tensors of one dtype."""
    l = x_lab[:, 0:1] + L_OFFSET
    a = x_lab[:, 1:2]
    b = x_lab[:, 2:3]
    a_predict = x_lab_predict[:, 1:2]
    b_predict = x_lab_predict[:, 2:3]
    local_l = find_local_patch(l, patch_size)
    local_a = find_local_patch(a, patch_size)
    local_b = find_local_patch(b, patch_size)
    local_a_predict = find_local_patch(a_predict, patch_size)
    local_b_predict = find_local_patch(b_predict, patch_size)
    local_color_difference = (local_l - l) ** 2 + (local_a - a) ** 2 + (local_b - b) ** 2
    correlation = F.softmax(-1 * local_color_difference / alpha, dim=1)
    return torch.cat((torch.sum(correlation * local_a_predict, dim=1, keepdim=True),
                      torch.sum(correlation * local_b_predict, dim=1, keepdim=True)), 1)


def weighted_average_color(x_lab, x_lab_predict, patch_size=3, alpha=1, scale_factor=1, dtype=torch.float64):
    """The reference's forward on CPU tensors, the arithmetic in `dtype`."""
    x_lab = F.interpolate(x_lab.detach().cpu().float(), scale_factor=scale_factor)
    return compose(x_lab.to(dtype), x_lab_predict.detach().cpu().float().to(dtype), patch_size, alpha)


def gradients(x_lab, x_lab_predict, G, patch_size=3, alpha=1, scale_factor=1, dtype=torch.float64):
    """Autograd of the composition for an incoming G: (y, d x_lab, d x_lab_predict), the gradients in the inputs' full
    shapes (x_lab's at its own, un-resized size), everything in `dtype`."""
    x = x_lab.detach().cpu().float().to(dtype).requires_grad_(True)
    p = x_lab_predict.detach().cpu().float().to(dtype).requires_grad_(True)
    y = compose(F.interpolate(x, scale_factor=scale_factor), p, patch_size, alpha)
    dx, dp = torch.autograd.grad(y, (x, p), G.detach().cpu().to(dtype))
    return y.detach(), dx, dp
