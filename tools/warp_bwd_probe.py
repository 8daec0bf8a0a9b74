#!/usr/bin/env python
"""WarpNet's training path behind the trunk tensor at 216x384 inputs (54x96 maps), N = 8 and N = 1, synthetic weights, seeded
output gradients.

Prints the GPU time (HIP events, launch queue primed, every shape warmed; p10 / median / p90 over the rounds) and peak device
memory on top of the forward of
  * the no-grad forward (heads frozen, trunk tensors given),
  * the forward that saves what the backward needs (WarpNet._train_from_trunks),
  * the backward of that (all 19 parameter gradients), and the same with the seam gradient,
  * the 1x1 weight-gradient kernel alone, with its share of the fp32 MFMA peak,
next to the torch composition of the same sub-network (the oracle's functions on the device in fp32, vendor convolutions,
forward + backward), timed in the same call, alternating with the HIP path.

    python tools/warp_bwd_probe.py              # the table
    python tools/warp_bwd_probe.py --hip-only   # 1 warm-up + 5 training steps at N = 1 (for a rocprofv3 --kernel-trace --stats run)
"""
import functools
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dvc_amd import ops, synth  # noqa: E402
from models.NonlocalNet import WarpNet  # noqa: E402
from oracle import dvc_oracle as O  # noqa: E402
import probe_timing  # noqa: E402
from probe_timing import peak_mem, spread  # noqa: E402

PEAK = 157.3e12     # fp32 MFMA, MI355X
h, w, T = 54, 96, 0.01
dev = torch.device("cuda")
device_time = functools.partial(probe_timing.device_time, warm=False)     # (run() warms every shape itself)


def fmt(name, samples):
    p10, med, p90 = spread(samples)
    return f"  {name:44s} p10 {p10:8.3f}  median {med:8.3f}  p90 {p90:8.3f} ms"


def make(N):
    net = WarpNet(1)
    net.load_state_dict(synth.warpnet_state_dict(0))
    for name in ("layer2_1", "layer3_1", "layer4_1", "layer5_1"):
        for p in getattr(net, name).parameters():
            p.requires_grad = False
    net.train().cuda()
    g = torch.Generator().manual_seed(0)
    tA = (torch.randn(N, 256, h, w, generator=g).abs() * 0.5).cuda()
    tB = (torch.randn(N, 256, h, w, generator=g).abs() * 0.5).cuda()
    blab = (torch.randn(N, 3, h, w, generator=g) * 30).cuda()
    gy = torch.randn(N, 3, 4 * h, 4 * w, generator=g).cuda()
    gs = torch.randn(N, 1, 4 * h, 4 * w, generator=g).cuda()
    return net, tA, tB, blab, gy, gs


def torch_composition(sd, tA, tB, blab_map, gy, gs):
    """The oracle's functions on the device, fp32, autograd forward + backward (P x P matrices and all)."""
    fa, fb = tA, tB
    for b in range(3):
        fa, fb = O.residual_block(sd, f"layer.{b}", fa), O.residual_block(sd, f"layer.{b}", fb)
    theta, phi = O.corr_project(sd, "theta", fa), O.corr_project(sd, "phi", fb)
    y, sim, _ = O.correlate(theta, phi, blab_map, T)
    y = F.interpolate(y, scale_factor=4, mode="nearest")
    sim = F.interpolate(sim, scale_factor=4, mode="nearest")
    return (y * gy).sum() + (sim * gs).sum()


def run(N, rounds=7):
    net, tA, tB, blab, gy, gs = make(N)
    params = [p for _, p in net._trunk_named_parameters()]
    sd = {k: v for k, v in net.named_parameters()}
    blab_map = F.interpolate(blab, scale_factor=4, mode="nearest")     # avg_pool2d(., 4) of it is blab again

    def fwd_nograd():
        with torch.no_grad():
            fa, fb = net._trunk(tA), net._trunk(tB)
            th, ph = net.project("theta", fa), net.project("phi", fb)
            return ops.corr_fwd(th, ph, blab.view(N, 3, -1), T, h, w)

    def fwd_saving():
        return net._train_from_trunks(tA, tB, blab, T)

    state = {}

    def prep():
        y, sim = fwd_saving()
        state["loss"] = (y * gy).sum() + (sim * gs).sum()

    def bwd():
        torch.autograd.grad(state["loss"], params, retain_graph=True)

    def comp_step():
        torch.autograd.grad(torch_composition(sd, tA, tB, blab_map, gy, gs), params)

    def hip_step():
        y, sim = fwd_saving()
        torch.autograd.grad((y * gy).sum() + (sim * gs).sum(), params)

    for fn in (fwd_nograd, fwd_saving, prep, bwd, hip_step, comp_step):      # every shape warmed, every pack made
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ("fwd_nograd", "fwd_saving", "bwd", "hip_step", "comp_step")}
    for _ in range(rounds):
        t["fwd_nograd"].append(device_time(fwd_nograd, 3))
        t["fwd_saving"].append(device_time(fwd_saving, 3))
        prep()
        t["bwd"].append(device_time(bwd, 3))
        t["hip_step"].append(device_time(hip_step, 2))
        t["comp_step"].append(device_time(comp_step, 2))
    print(f"N = {N}  (maps {h}x{w}, inputs {4 * h}x{4 * w}, T = {T})")
    print(fmt("no-grad forward (trunk, projections, corr)", t["fwd_nograd"]))
    print(fmt("saving forward", t["fwd_saving"]))
    print(fmt("backward (19 parameter gradients)", t["bwd"]))
    print(fmt("HIP forward + backward", t["hip_step"]))
    print(fmt("torch composition forward + backward", t["comp_step"]))
    # the 1x1 weight-gradient kernel alone
    dT, Fin = torch.randn(N, 256, h * w, device=dev), torch.randn(N, 256, h * w, device=dev)
    ops.warp_k1_wgrad(dT, Fin)
    k1 = [device_time(lambda: ops.warp_k1_wgrad(dT, Fin), 10) for _ in range(rounds)]
    flops = 2.0 * 256 * 256 * N * h * w
    print(fmt("dvc_warp_k1_wgrad 256x256, K = N*P", k1) + f"   {flops / (statistics.median(k1) * 1e-3) / PEAK:.3f} of the fp32 MFMA peak")
    # peak memory on top of what is live before the call
    for name, fn in (("saving forward + backward", hip_step), ("torch composition", comp_step)):
        print(f"  peak memory, {name:32s} {peak_mem(fn):9.1f} MiB")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    if "--hip-only" in sys.argv:
        net, tA, tB, blab, gy, gs = make(1)
        params = [p for _, p in net._trunk_named_parameters()]
        for _ in range(6):
            y, sim = net._train_from_trunks(tA, tB, blab, T)
            torch.autograd.grad((y * gy).sum() + (sim * gs).sum(), params)
        torch.cuda.synchronize()
    else:
        for N in (8, 1):
            run(N)
