#!/usr/bin/env python
"""VGG19's input gradient at the training crop: x [16, 3, 216, 384], keys r12 r22 r32 r42 r52 (train.py:649-668), seeded
random output gradients, synthetic weights.

Prints the GPU time (HIP events, launch queue primed, median of rounds), the FLOPs computed from shapes, TFLOP/s and share of
the fp32 MFMA peak (of HBM bandwidth for the elementwise tensor_lab2rgb) and the peak device memory of
  * the no-grad forward,
  * the forward that saves the post-ReLU activations (grad mode),
  * the backward (VGG19_pytorch._input_grad: the layers in reverse),
  * tensor_lab2rgb forward + backward,
then the torch composition on the device (oracle.vgg19_forward under autograd, vendor convolutions) as a yardstick only.

    python tools/vgg_bwd_probe.py              # the table
    python tools/vgg_bwd_probe.py --hip-only   # only this library's forward + backward (for a rocprofv3 --kernel-trace --stats run)
"""
import contextlib
import functools
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402

from dvc_amd import arch, ops, synth  # noqa: E402
from models.NonlocalNet import VGG19_pytorch  # noqa: E402
from oracle import dvc_oracle as O  # noqa: E402
import probe_timing  # noqa: E402
from probe_timing import peak_mem  # noqa: E402
from utils.util import tensor_lab2rgb  # noqa: E402

PEAK = 157.3e12     # fp32 MFMA, MI355X
HBM = 8.0e12        # HBM3E peak, MI355X
B, H, W = 16, 216, 384
KEYS = ["r12", "r22", "r32", "r42", "r52"]
ITERS = 10
dev = torch.device("cuda")
median_time = functools.partial(probe_timing.median_time, rounds=5)


def conv_flops(keys):
    """2 * MACs of the 3x3 convolutions up to the deepest key (the backward's input-gradient convolutions have the same count:
    the forward's shapes mirrored; conv1_1's has 3 output channels where the forward has 3 input channels)."""
    last = max(arch.VGG_KEYS.index(k) for k in keys)
    h, w, fl = H, W, 0.0
    convs = iter(arch.VGG_CONVS)
    for key in arch.VGG_KEYS[:last + 1]:
        if key[0] == "p":
            h, w = h // 2, w // 2
        else:
            _, ci, co = next(convs)
            fl += 2.0 * B * h * w * ci * co * 9
    return fl


def main():
    with contextlib.redirect_stdout(io.StringIO()):
        m = VGG19_pytorch()
    m.load_state_dict(synth.vgg19_state_dict(0))
    for p in m.parameters():
        p.requires_grad = False
    m.eval().cuda()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, H, W, generator=g).to(dev)
    with torch.no_grad():
        shapes = [o.shape for o in m(x, KEYS)]
    G = {k: torch.randn(s, generator=g).to(dev) for k, s in zip(KEYS, shapes)}

    def fwd_saved():
        saved = {}
        m._forward(x, KEYS, True, False, saved=saved)
        return saved

    saved = fwd_saved()

    def bwd():
        return m._input_grad(saved, G, True)

    lab = torch.cat((torch.rand(B, 1, H, W, generator=g) * 100, torch.rand(B, 2, H, W, generator=g) * 200 - 100), 1).to(dev)
    grgb = torch.randn(B, 3, H, W, generator=g).to(dev)

    def lab_fb():
        return ops.lab2rgb(lab), ops.lab2rgb_bwd(lab, grgb)

    if "--hip-only" in sys.argv:
        # warm-up: packs the backward filters (one-time torch flips / copies in the cache), then ITERS training-style steps on
        # fresh leaves (no clone, no gradient accumulation): every kernel the steady state launches is one of this library's
        xg, li = x.detach().requires_grad_(True), lab.detach().requires_grad_(True)
        torch.autograd.backward(m(xg, KEYS), [G[k] for k in KEYS])
        tensor_lab2rgb(li).backward(grgb)
        torch.cuda.synchronize()
        for _ in range(ITERS):
            xg, li = x.detach().requires_grad_(True), lab.detach().requires_grad_(True)
            torch.autograd.backward(m(xg, KEYS), [G[k] for k in KEYS])
            tensor_lab2rgb(li).backward(grgb)
        torch.cuda.synchronize()
        print(f"hip-only: 1 warm-up + {ITERS} forward + backward steps done")
        return

    fl = conv_flops(KEYS)
    print(f"VGG19 input gradient, x [{B}, 3, {H}, {W}], keys {' '.join(KEYS)}; {torch.cuda.get_device_name(0)}")
    print(f"3x3 convolutions to r52: {fl / 1e9:.1f} GFLOP forward, {fl / 1e9:.1f} GFLOP backward ({fl / B / 1e9:.1f} per image), "
          "counted as direct convolutions (the Winograd layers execute fewer: a rate above 1.0 of peak is possible)")
    with torch.no_grad():
        t_nf = median_time(lambda: m(x, KEYS), 3)
        mem_nf = peak_mem(lambda: m(x, KEYS))
    t_fs = median_time(fwd_saved, 3)
    mem_fs = peak_mem(fwd_saved)
    t_b = median_time(bwd, 3)
    mem_b = peak_mem(bwd)
    for nm, t, mem in (("no-grad forward", t_nf, mem_nf), ("forward, activations saved", t_fs, mem_fs), ("backward (d x)", t_b, mem_b)):
        print(f"{nm:28s} {t:8.3f} ms  {fl / t / 1e9:6.1f} TFLOP/s direct-equivalent = {fl / t / 1e9 / (PEAK / 1e12):.3f} of fp32 MFMA peak; "
              f"peak memory {mem:8.1f} MiB")
    print(f"backward / no-grad forward: {t_b / t_nf:.2f}x")
    t_l = median_time(lab_fb, 10)
    byts = 4.0 * B * H * W * (3 + 3 + 6 + 3)
    print(f"{'tensor_lab2rgb fwd + bwd':28s} {t_l:8.3f} ms  {byts / 1e6:.1f} MB moved -> {byts / t_l / 1e9:.2f} TB/s = "
          f"{byts / t_l / 1e9 / (HBM / 1e12):.3f} of HBM peak; peak memory {peak_mem(lab_fb):8.1f} MiB")

    # yardstick: the torch composition on the device (vendor convolutions), forward + backward through p5 as the oracle runs
    sd = {k: v.to(dev) for k, v in synth.vgg19_state_dict(0).items()}
    Gl = [G[k] for k in KEYS]

    def torch_fb():
        xr = x.clone().requires_grad_(True)
        outs = O.vgg19_forward(sd, xr, KEYS)
        torch.autograd.backward(outs, Gl)
        return xr.grad

    t_t = median_time(torch_fb, 2, rounds=3)
    mem_t = peak_mem(torch_fb)
    xr = x.clone().requires_grad_(True)
    outs = m(xr, KEYS)
    torch.autograd.backward(outs, Gl)
    ref = torch_fb()
    d = ((xr.grad - ref).norm() / ref.norm()).item()
    print(f"torch composition fwd + bwd  {t_t:8.3f} ms (HIP fwd-saved + bwd {t_fs + t_b:.3f} ms), peak memory {mem_t:8.1f} MiB; "
          f"rel L2 |HIP dx - torch dx| {d:.2e}")


if __name__ == "__main__":
    main()
