#!/usr/bin/env python
"""WarpNet's whole training step — heads, trunk, projections, correlation — at 216x384 inputs, N = 1 and N = 2, synthetic
weights, random normalised feature maps, seeded output gradients.

Prints the GPU time (HIP events, launch queue primed, every shape warmed; p10 / median / p90 over the rounds) and the peak device
memory of forward + backward of
  * the 19-gradient step (heads frozen: what the training path gives without WarpNet.set_head_training),
  * the 43-gradient step (set_head_training(True), nothing frozen),
  * the 43-gradient step with the trunk frozen (heads only),
  * the torch composition of the oracle's WarpNet on the device in fp32 (vendor convolutions, autograd, all 43 gradients),
timed in the same call, alternating.

    python tools/warp_heads_probe.py              # the table
    python tools/warp_heads_probe.py --hip-only   # 1 warm-up + 5 steps of the 43-gradient step at N = 1 (for a kernel trace)
"""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402

from dvc_amd import ops, synth  # noqa: E402
from models.NonlocalNet import WarpNet  # noqa: E402
from oracle import dvc_oracle as O  # noqa: E402
import probe_timing  # noqa: E402
from probe_timing import peak_mem, spread  # noqa: E402

H, W, T = 216, 384, 0.01
HEADS = ("layer2_1", "layer3_1", "layer4_1", "layer5_1")
device_time = functools.partial(probe_timing.device_time, warm=False)     # (run() warms every shape itself)


def fmt(name, samples):
    p10, med, p90 = spread(samples)
    return f"  {name:52s} p10 {p10:8.3f}  median {med:8.3f}  p90 {p90:8.3f} ms"


def make_net(head_training, frozen=()):
    net = WarpNet(1)
    net.load_state_dict(synth.warpnet_state_dict(0))
    for n, p in net.named_parameters():
        if n.split(".")[0] in frozen:
            p.requires_grad = False
    return net.set_head_training(head_training).train().cuda()


def make_inputs(N):
    g = torch.Generator().manual_seed(0)
    lab = (torch.randn(N, 3, H, W, generator=g) * 30).cuda()
    feats = [ops.channel_l2norm(torch.randn(N, c, H // s, W // s, generator=g).abs().cuda())
             for c, s in ((128, 2), (256, 4), (512, 8), (512, 16))] * 2
    gy, gs = torch.randn(N, 3, H, W, generator=g).cuda(), torch.randn(N, 1, H, W, generator=g).cuda()
    return [lab] + feats, gy, gs


def hip_step(net, ins, gy, gs):
    params = [p for p in net.parameters() if p.requires_grad]

    def step():
        y, sim = net(*ins, temperature=T)
        return torch.autograd.grad((y * gy).sum() + (sim * gs).sum(), params)
    return step


def run(N, rounds=7):
    ins, gy, gs = make_inputs(N)
    steps = {
        "HIP, 19 gradients (heads frozen)": hip_step(make_net(False, frozen=HEADS), ins, gy, gs),
        "HIP, 43 gradients (set_head_training)": hip_step(make_net(True), ins, gy, gs),
        "HIP, 24 gradients (heads only, trunk frozen)": hip_step(make_net(True, frozen=("layer", "theta", "phi")), ins, gy, gs),
    }
    sd = {k: v.detach().clone().cuda().requires_grad_() for k, v in synth.warpnet_state_dict(0).items()}

    def comp_step():
        y, sim = O.warpnet_forward(sd, *ins, temperature=T)
        return torch.autograd.grad((y * gy).sum() + (sim * gs).sum(), list(sd.values()))
    steps["torch composition, 43 gradients"] = comp_step

    for fn in steps.values():      # every shape warmed, every pack made
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in steps}
    for _ in range(rounds):
        for k, fn in steps.items():
            t[k].append(device_time(fn, 2))
    print(f"N = {N}  (inputs {H}x{W}, T = {T}; forward + backward)")
    for k in steps:
        print(fmt(k, t[k]))
    for k, fn in steps.items():
        print(f"  peak memory, {k:46s} {peak_mem(fn):9.1f} MiB")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU"
    torch.manual_seed(0)
    if "--hip-only" in sys.argv:
        ins, gy, gs = make_inputs(1)
        step = hip_step(make_net(True), ins, gy, gs)
        for _ in range(6):
            step()
        torch.cuda.synchronize()
    else:
        for N in (1, 2):
            run(N)
