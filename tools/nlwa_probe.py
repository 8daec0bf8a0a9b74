#!/usr/bin/env python
"""NonlocalWeightedAverage at the benchmark shape: x_lab [B, 3, 216, 384], scale_factor 0.25 -> 54 x 96 (N = 5184),
feature [B, 128, 108, 192], patch_size 3 (K = 1152), alpha 0.5.

Prints, for B = 1 and B = 16, the fused op's GPU time (HIP events, launch queue primed, median of rounds) and its fraction
of the fp32 MFMA peak on the direct formulation's 2 N^2 K flop, then the time and peak device memory of the reference's own
torch composition (F.unfold + bmm + softmax + bmm, models/NonlocalNet.py:86-111) on the same inputs.

    python tools/nlwa_probe.py                 # the table
    python tools/nlwa_probe.py --fused-only    # only the fused op's launches (for a rocprofv3 --kernel-trace --stats run)
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dvc_amd import _lib  # noqa: E402
from models.NonlocalNet import NonlocalWeightedAverage  # noqa: E402

PEAK = 157.3e12     # fp32 MFMA, MI355X
H, W, SF, K3, C, ALPHA = 216, 384, 0.25, 3, 128, 0.5
N = (H // 4) * (W // 4)
KDIM = C * K3 * K3
dev = torch.device("cuda")
_filler = None


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, 3, H, W, generator=g) * 220 - 110).to(dev)
    f = (torch.randn(B, C, H // 2, W // 2, generator=g) * (6.0 * ALPHA / KDIM) ** 0.5).to(dev)
    return x, f


def device_time(fn, reps):
    """ms per call with the launch queue primed (filler GEMMs enqueued first: the events bracket kernel execution only)."""
    global _filler
    if _filler is None:
        _filler = (torch.randn(8192, 8192, device=dev), torch.randn(8192, 8192, device=dev), torch.empty(8192, 8192, device=dev))
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2 + reps):
        torch.mm(_filler[0], _filler[1], out=_filler[2])
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def median_time(fn, reps, rounds=7):
    return statistics.median(device_time(fn, reps) for _ in range(rounds))


def composition(x_lab, feature):
    """The reference's forward, op for op (models/NonlocalNet.py:86-111 with find_local_patch :12-17)."""
    x_lab = F.interpolate(x_lab, scale_factor=SF)
    B, _, h, w = x_lab.shape
    feature = F.interpolate(feature, size=(h, w))
    x_ab = x_lab[:, 1:3].detach()
    U = F.unfold(feature, kernel_size=(K3, K3), padding=(K3 // 2, K3 // 2), stride=(1, 1)).view(B, -1, h * w)
    A = torch.softmax(torch.matmul(U.permute(0, 2, 1), U) / ALPHA, dim=-1)
    return torch.matmul(A, x_ab.reshape(B, 2, -1).permute(0, 2, 1)).permute(0, 2, 1).contiguous().view(B, 2, h, w)


def peak_mem(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    m = NonlocalWeightedAverage()
    if "--fused-only" in sys.argv:
        with torch.no_grad():
            for B in (1, 16):
                x, f = inputs(B)
                for _ in range(5):
                    m(x, f, K3, ALPHA, SF)
        torch.cuda.synchronize()
        print("fused-only launches done")
        return
    print(f"NonlocalWeightedAverage, 54x96 (N = {N}), K = {KDIM}, alpha = {ALPHA}; {torch.cuda.get_device_name(0)}")
    with torch.no_grad():
        for B in (1, 16):
            x, f = inputs(B)
            fl = 2.0 * N * N * KDIM * B
            reps = 40 if B == 1 else 5
            t_f = median_time(lambda: m(x, f, K3, ALPHA, SF), reps)
            mem_f = peak_mem(lambda: m(x, f, K3, ALPHA, SF))
            t_c = median_time(lambda: composition(x, f), max(2, reps // 4), rounds=5)
            mem_c = peak_mem(lambda: composition(x, f))
            d = (m(x, f, K3, ALPHA, SF) - composition(x, f)).abs().max().item()
            ws = _lib.load().dvc_nlwa_workspace_bytes(B, C, K3, H // 4, W // 4) / 2**20
            print(f"B={B:2d}: fused {t_f:8.3f} ms  {fl / 1e9:7.1f} GFLOP direct -> {fl / t_f / 1e9:6.1f} TFLOP/s = "
                  f"{fl / t_f / 1e9 / (PEAK / 1e12):.3f} of fp32 MFMA peak; memory: workspace {ws:.1f} MiB + "
                  f"{mem_f:.1f} MiB per call")
            print(f"       torch composition {t_c:8.3f} ms ({t_c / t_f:.2f}x), peak memory {mem_c:8.1f} MiB; "
                  f"max |fused - composition| {d:.2e}")


if __name__ == "__main__":
    main()
