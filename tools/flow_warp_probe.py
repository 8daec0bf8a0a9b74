#!/usr/bin/env python
"""WarpingLayer at the training frame: x [B, 3, 216, 384] warped by flow [B, 2, 216, 384] ~ N(0, 4 px), align_corners=False
(what train.py's consistent_loss_fn runs), for B = 1 and B = 16.

Prints the GPU time (HIP events, launch queue primed; p10 / median / p90 over rounds that alternate between the two
implementations) of the HIP forward (dvc_flow_warp_fwd) and of forward + backward to x only (train.py's flow carries no
gradient: workspace memset, amax, integer scatter, finish), the same for the torch composition of the reference's forward
(get_grid, the division, F.grid_sample, autograd) on the device, the peak memory of both, and the rate of the backward's
64-bit integer atomics: 8 B x 4 corners x B C H W added bytes over the time of the whole backward call (so a lower bound of
what the scatter launch itself achieves).  Writes the same lines to profiles/flow_warp_probe.txt.

    python tools/flow_warp_probe.py
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dvc_amd import _lib  # noqa: E402
from utils.warping import WarpingLayer, get_grid  # noqa: E402

C, H, W = 3, 216, 384
ROUNDS = 9
OUT = os.path.join(ROOT, "profiles", "flow_warp_probe.txt")
dev = torch.device("cuda")
_filler = None
_lines = []


def say(line):
    print(line, flush=True)
    _lines.append(line)


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, H, W, generator=g) * 50).to(dev)
    flow = (torch.randn(B, 2, H, W, generator=g) * 4).to(dev)
    G = torch.randn(B, C, H, W, generator=g).to(dev)
    return x, flow, G


def device_time(fn, reps):
    """ms per call with the launch queue primed (filler GEMMs enqueued first: the events bracket kernel execution only)."""
    global _filler
    if _filler is None:
        _filler = (torch.randn(8192, 8192, device=dev), torch.randn(8192, 8192, device=dev), torch.empty(8192, 8192, device=dev))
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(8):
        torch.mm(_filler[0], _filler[1], out=_filler[2])
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(ts):
    ts = sorted(ts)
    q = lambda f: ts[min(len(ts) - 1, int(round(f * (len(ts) - 1))))]  # noqa: E731
    return q(0.1), q(0.5), q(0.9)


def composition(x, flow):
    """The reference's forward, op for op (get_grid on the device)."""
    flow_for_grip = torch.zeros_like(flow)
    flow_for_grip[:, 0, :, :] = flow[:, 0, :, :] / ((flow.size(3) - 1.0) / 2.0)
    flow_for_grip[:, 1, :, :] = flow[:, 1, :, :] / ((flow.size(2) - 1.0) / 2.0)
    grid = (get_grid(x) + flow_for_grip).permute(0, 2, 3, 1)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def peak_mem(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def main():
    m = WarpingLayer()
    lib = _lib.load()
    say(f"WarpingLayer, [B, {C}, {H}, {W}], flow ~ N(0, 4 px), align_corners=False; {torch.cuda.get_device_name(0)}; "
        f"p10 / median / p90 of {ROUNDS} alternating rounds, GPU ms per call")
    for B in (1, 16):
        x, flow, G = inputs(B)
        xg = x.clone().requires_grad_(True)
        reps = 40 if B == 1 else 10

        def fwd(layer):
            with torch.no_grad():
                return layer(x, flow)

        def fwd_bwd(layer):
            xg.grad = None
            layer(xg, flow).backward(G)

        nbytes = lib.dvc_flow_warp_bwd_workspace_bytes(B, C, H, W)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        dx = torch.empty_like(x)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

        def bwd_call():
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.dvc_flow_warp_bwd(p(x), p(flow), p(G), B, C, H, W, 0, p(dx), None, p(ws), nbytes, stream),
                       "dvc_flow_warp_bwd")

        t = {key: [] for key in ("hip fwd", "torch fwd", "hip fwd+bwd", "torch fwd+bwd", "hip bwd call")}
        for _ in range(ROUNDS):
            t["hip fwd"].append(device_time(lambda: fwd(m), reps))
            t["torch fwd"].append(device_time(lambda: fwd(composition), reps))
            t["hip fwd+bwd"].append(device_time(lambda: fwd_bwd(m), reps))
            t["torch fwd+bwd"].append(device_time(lambda: fwd_bwd(composition), reps))
            t["hip bwd call"].append(device_time(bwd_call, reps))
        mem = {"hip fwd": peak_mem(lambda: fwd(m)), "torch fwd": peak_mem(lambda: fwd(composition)),
               "hip fwd+bwd": peak_mem(lambda: fwd_bwd(m)), "torch fwd+bwd": peak_mem(lambda: fwd_bwd(composition))}
        d = (fwd(m) - fwd(composition)).abs().max().item()
        for key, ts in t.items():
            lo, med, hi = spread(ts)
            line = f"B={B:2d}  {key:14s} {lo:8.4f} / {med:8.4f} / {hi:8.4f} ms"
            if key in mem:
                line += f"   peak memory {mem[key]:8.1f} MiB"
            else:
                added = 8.0 * 4 * B * C * H * W
                line += f"   dx only: {added / 1e6:6.1f} MB of 64-bit integer adds -> >= {added / med / 1e6:7.1f} GB/s"
            say(line)
        for a, b in (("hip fwd", "torch fwd"), ("hip fwd+bwd", "torch fwd+bwd")):
            fa, fb = spread(t[a]), spread(t[b])
            say(f"B={B:2d}  {b} / {a}: {fb[1] / fa[1]:.2f}x at the medians; hip median {fa[1]:.4f} ms "
                f"{'<' if fa[1] < fb[0] else '>='} torch p10 {fb[0]:.4f} ms")
        say(f"B={B:2d}  max |hip - composition| {d:.2e} (max |x| {x.abs().max().item():.1f})")
    with open(OUT, "w") as f:
        f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
