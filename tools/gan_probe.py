#!/usr/bin/env python
"""Discriminator_x64 as a frozen critic at the training frame: forward + input gradient at 216 x 384, ndf = 64, batch 16.

Prints the GPU time (HIP events around whole calls; p10 / median / p90 over rounds that alternate between the two
implementations) of dvc_amd.gan.Discriminator_x64 and of the same network composed from torch ops on the same device
(F.conv2d on W_bar / sigma with the power step in torch, softmax attention, autograd), the peak memory of both on top of what
is resident before the call, and per 4x4 stride-2 layer the time of the forward launch (dvc_gan_conv4s2) and of its input
gradient (dvc_gan_conv4s2_dgrad) with the achieved share of the 157.3 TFLOP/s fp32 matrix peak.  The per-layer figures are CALL
times — events around 20 back-to-back calls of the Python wrapper (descriptor, torch.empty, ctypes call, launch) — not kernel
times from a trace: where the host's enqueue gap exceeds a short kernel it is part of the number, so the shares are lower bounds
of what the kernels reach.  Writes the same lines to profiles/gan_probe.txt.

    python tools/gan_probe.py
    python tools/gan_probe.py --train

--train: the module after set_parameter_training() against the autograd composition of tests/gan_train_reference.py on the
device in float32 — train.py's discriminator step (zero_grad, two forwards on detached pairs, the relativistic least-squares
loss, one backward into the 21 parameters) and the generator step of an unfrozen module (one forward, backward into the
parameters AND the input); then per layer the call time of the new weight gradient (dvc_gan_conv4s2_wgrad, slot sum included).
Its lines go under the frozen-critic block of profiles/gan_probe.txt, which it leaves as it is.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dvc_amd import arch, ops, synth  # noqa: E402
from dvc_amd.gan import Discriminator_x64  # noqa: E402

N, H, W, NDF = 16, 216, 384, 64
ROUNDS, REPS = 7, 10
PEAK = 157.3
OUT = os.path.join(ROOT, "profiles", "gan_probe.txt")
dev = torch.device("cuda")
_lines = []


def say(line):
    print(line, flush=True)
    _lines.append(line)


def timed(fn, reps=REPS):
    """ms per call, events around `reps` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pct(v):
    v = sorted(v)
    return v[len(v) // 10], v[len(v) // 2], v[(9 * len(v)) // 10]


def torch_step(sd, x, g_out, g_f4):
    """The reference's arithmetic from torch ops; u / v are updated in place in `sd` as the reference does."""
    def sn(prefix):
        w, u, v = sd[prefix + ".weight_bar"], sd[prefix + ".weight_u"], sd[prefix + ".weight_v"]
        Wm = w.view(w.shape[0], -1)
        v.copy_(F.normalize(Wm.t() @ u, dim=0, eps=1e-12))
        u.copy_(F.normalize(Wm @ v, dim=0, eps=1e-12))
        return w / (u @ (Wm @ v)), sd[prefix + ".bias"]
    x = x.detach().requires_grad_(True)
    a = x
    for name in arch.GAN_LAYERS:
        a = F.leaky_relu(F.conv2d(a, *sn(name + ".0.module"), 2, 1), 0.2)
        if name == arch.GAN_ATTENTION_AFTER:
            f4 = a
            n, c, h, w = a.shape
            q, k, v = (F.conv2d(a, *sn(f"attention.{m}.module")).view(n, c, h * w) for m in arch.GAN_ATTENTION_CONVS)
            att = torch.softmax(torch.bmm(q.transpose(1, 2), k), -1)
            a = sd["attention.gamma"] * torch.bmm(v, att.transpose(1, 2)).view(n, c, h, w) + a
    out = F.conv2d(a, *sn("last.module")).mean((2, 3)).view(-1, 1)
    torch.autograd.backward([out, f4], [g_out, g_f4])
    return x.grad


TRAIN_MARK = "Discriminator_x64 training"


def write_block(train):
    """The frozen-critic block first, the --train block under it; a run replaces its own block only."""
    old = open(OUT).read().split("\n") if os.path.exists(OUT) else []
    cut = next((i for i, line in enumerate(old) if line.startswith(TRAIN_MARK)), len(old))
    frozen, trained = [line for line in old[:cut] if line], [line for line in old[cut:] if line]
    with open(OUT, "w") as f:
        f.write("\n".join((frozen + _lines) if train else (_lines + trained)) + "\n")


def compare(title, impls):
    """Warm up, peak memory, then ROUNDS rounds that alternate between the implementations; one line each and the ratio."""
    times, peaks = {n: [] for n, _ in impls}, {}
    for name, fn in impls:
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(ROUNDS):
        for name, fn in impls:
            times[name].append(timed(fn))
    for name, _ in impls:
        p10, med, p90 = pct(times[name])
        say(f"{name:6s} {title}: {p10:.3f} / {med:.3f} / {p90:.3f} ms (p10 / median / p90 of {ROUNDS} rounds x {REPS} calls), peak "
            f"memory on top of the resident tensors {peaks[name]:.0f} MiB")
    say(f"hip / torch at the median, {title}: {pct(times['hip'])[1] / pct(times['torch'])[1]:.2f}")


def main_train():
    import gan_train_reference as T
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    sd = synth.discriminator_state_dict(0, ndf=NDF)
    net = Discriminator_x64(ndf=NDF)
    net.load_state_dict(sd)
    net.to(dev).set_parameter_training()
    params, uv = T.leaf_params(sd, torch.float32, dev)
    real, fake = (torch.randn(N, 6, H, W, generator=g).to(dev) for _ in range(2))
    g_out, g_f4 = torch.randn(N, 1, generator=g).to(dev), torch.randn(N, 4 * NDF, H // 16, W // 16, generator=g).to(dev)

    def zero_torch():
        for p in params.values():
            p.grad = None

    def hip_d():
        net.zero_grad(set_to_none=True)
        T.relativistic_ls_loss(net(real.detach())[0], net(fake.detach())[0]).backward()

    def torch_d():
        zero_torch()
        T.relativistic_ls_loss(T.autograd_forward(params, uv, real.detach())[0], T.autograd_forward(params, uv, fake.detach())[0]).backward()

    def hip_g():
        net.zero_grad(set_to_none=True)
        torch.autograd.backward(list(net(real.detach().requires_grad_(True))), [g_out, g_f4])

    def torch_g():
        zero_torch()
        torch.autograd.backward(list(T.autograd_forward(params, uv, real.detach().requires_grad_(True))), [g_out, g_f4])

    say(f"{TRAIN_MARK} (set_parameter_training, all 21 parameters hot), {N} x 6 x {H} x {W}, ndf {NDF}, "
        f"{torch.cuda.get_device_name(0)}")
    compare("discriminator step (2 forwards + 1 backward, inputs detached)", (("hip", hip_d), ("torch", torch_d)))
    compare("forward + backward to parameters and input", (("hip", hip_g), ("torch", torch_g)))
    # per layer: the weight-gradient call alone (the MFMA launch and the slot sum)
    a, inv = real, torch.ones(1, device=dev)
    for name, cin, cout in arch.gan_conv_plan(6, NDF):
        m = getattr(net, name)[0].module
        y = ops.gan_conv4s2(a, m.weight_bar.detach(), m.bias.detach(), inv)
        dz = torch.randn_like(y)
        hw = tuple(a.shape[2:])
        flops = 2.0 * N * cout * cin * 16 * y.shape[2] * y.shape[3]
        S = ops.gan_conv4s2_wgrad_splits(N, cin, hw[0], hw[1], cout)
        tw = sorted(timed(lambda: ops.gan_conv4s2_wgrad(dz, a), 20) for _ in range(ROUNDS))[ROUNDS // 2]
        say(f"{name}: {cin:4d} -> {cout:4d} at {hw[0]:3d} x {hw[1]:3d}  {flops / 1e9:6.2f} GFLOP  S = {S:3d}  wgrad call {tw:7.3f} ms = "
            f"{100 * flops / tw / 1e9 / PEAK:5.1f} % of the fp32 matrix peak")
        a = y
    write_block(train=True)


def main():
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    sd = {k: v.to(dev) for k, v in synth.discriminator_state_dict(0, ndf=NDF).items()}
    net = Discriminator_x64(ndf=NDF)
    net.load_state_dict(sd)
    net.to(dev).requires_grad_(False)
    x = torch.randn(N, 6, H, W, generator=g).to(dev)
    g_out, g_f4 = torch.randn(N, 1, generator=g).to(dev), torch.randn(N, 4 * NDF, H // 16, W // 16, generator=g).to(dev)

    def hip_step():
        xd = x.detach().requires_grad_(True)
        out, f4 = net(xd)
        torch.autograd.backward([out, f4], [g_out, g_f4])
        return xd.grad

    def ref_step():
        return torch_step(sd, x, g_out, g_f4)

    say(f"Discriminator_x64 forward + input gradient, {N} x 6 x {H} x {W}, ndf {NDF}, {torch.cuda.get_device_name(0)}")
    times, peaks = {"hip": [], "torch": []}, {}
    for name, fn in (("hip", hip_step), ("torch", ref_step)):
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peaks[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(ROUNDS):
        for name, fn in (("hip", hip_step), ("torch", ref_step)):
            times[name].append(timed(fn))
    for name in ("hip", "torch"):
        p10, med, p90 = pct(times[name])
        say(f"{name:6s} forward + input backward: {p10:.3f} / {med:.3f} / {p90:.3f} ms (p10 / median / p90 of {ROUNDS} rounds x {REPS} "
            f"calls), peak memory on top of the resident tensors {peaks[name]:.0f} MiB")
    say(f"hip / torch at the median: {pct(times['hip'])[1] / pct(times['torch'])[1]:.2f}")

    # per layer: the forward launch and the input-gradient launch alone
    a, inv = x, torch.ones(1, device=dev)
    for name, cin, cout in arch.gan_conv_plan(6, NDF):
        m = getattr(net, name)[0].module
        wb, b = m.weight_bar.detach(), m.bias.detach()
        y = ops.gan_conv4s2(a, wb, b, inv)
        dz = torch.randn_like(y)
        hw = tuple(a.shape[2:])
        flops = 2.0 * N * cout * cin * 16 * y.shape[2] * y.shape[3]
        tf = sorted(timed(lambda: ops.gan_conv4s2(a, wb, b, inv), 20) for _ in range(ROUNDS))[ROUNDS // 2]
        tb = sorted(timed(lambda: ops.gan_conv4s2_dgrad(dz, wb, inv, hw, mask_act=a), 20) for _ in range(ROUNDS))[ROUNDS // 2]
        say(f"{name}: {cin:4d} -> {cout:4d} at {hw[0]:3d} x {hw[1]:3d}  {flops / 1e9:6.2f} GFLOP  forward call {tf:7.3f} ms = "
            f"{100 * flops / tf / 1e9 / PEAK:5.1f} % of the fp32 matrix peak   dgrad call {tb:7.3f} ms = {100 * flops / tb / 1e9 / PEAK:5.1f} %")
        a = y
    write_block(train=False)


if __name__ == "__main__":
    main_train() if "--train" in sys.argv[1:] else main()
