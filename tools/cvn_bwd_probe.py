#!/usr/bin/env python
"""ColorVidNet's training path at x [B, 7, 216, 384], B = 1 and 8, synthetic (contractive) weights, a seeded output gradient.

Prints the GPU time (HIP events, launch queue primed, median of rounds) and peak device memory of
  * the no-grad forward,
  * the forward that saves what the backward needs (ColorVidNet._forward(saved=...)),
  * the backward (ColorVidNet._backward: every parameter gradient and d x),
and the backward split into its weight-gradient launches (dvc_cvn_wgrad, each layer alone on its own shapes), its input-gradient
convolutions (ops.conv3x3 with the transposed filters, each layer alone) and the rest (head, InstanceNorm and ReLU backward),
with the weight-gradient kernel's share of the fp32 MFMA peak per layer class.

    python tools/cvn_bwd_probe.py              # the table
    python tools/cvn_bwd_probe.py --hip-only   # 1 warm-up + 5 training steps at B = 1 (for a rocprofv3 --kernel-trace --stats run)
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
from models.ColorVidNet import ColorVidNet  # noqa: E402
import probe_timing  # noqa: E402
from probe_timing import peak_mem  # noqa: E402

PEAK = 157.3e12     # fp32 MFMA, MI355X
H, W = 216, 384
dev = torch.device("cuda")
median_time = functools.partial(probe_timing.median_time, rounds=3)


def layer_shapes(B):
    """(conv entry, Cin, Cout, h, w of the output map) of the 30 3x3 layers at B x 216 x 384."""
    size = {"x": (H, W)}
    out = []
    for c in arch.CVN_CONVS:
        h, w = size[c["src"]]
        if c["pre"] == "norm_ss":
            h, w = (h + 1) // 2, (w + 1) // 2
        elif c["pre"] == "up":
            h, w = 2 * h, 2 * w
        size[c["dst"]] = (h, w)
        out.append((c, 7 if c["cin"] is None else c["cin"], c["cout"], h, w))
    return out


def main():
    with contextlib.redirect_stdout(io.StringIO()):
        m = ColorVidNet(7)
    m.load_state_dict(synth.colorvidnet_state_dict(0, contractive=True))
    m.cuda().train()
    g = torch.Generator().manual_seed(0)
    if "--hip-only" in sys.argv:
        x = (torch.rand(1, 7, H, W, generator=g) * 100 - 50).to(dev)
        gab = torch.randn(1, 2, H, W, generator=g).to(dev)
        for _ in range(6):
            m.zero_grad(set_to_none=True)
            m(x.requires_grad_(True)).backward(gab)
        torch.cuda.synchronize()
        return
    print(f"ColorVidNet training path, x [B, 7, {H}, {W}], contractive synthetic weights; {torch.cuda.get_device_name()}")
    for B in (1, 8):
        x = (torch.rand(B, 7, H, W, generator=g) * 100 - 50).to(dev)
        gab = torch.randn(B, 2, H, W, generator=g).to(dev)
        need = {n for n, _ in m.named_parameters()}
        fl = sum(2.0 * B * h * w * ci * co * 9 for _, ci, co, h, w in layer_shapes(B))

        def fwd():
            with torch.no_grad():
                return m(x)

        def fwd_saved():
            saved, rstd = {}, {}
            saved["ab"] = m._forward(x, saved=saved, rstd=rstd)
            return saved, rstd

        saved, rstd = fwd_saved()
        t = dict(saved)
        t.update({"rstd:" + k: v for k, v in rstd.items()})

        def bwd():
            return m._backward(t, gab, need, True)

        t_f, t_fs, t_b = median_time(fwd, 3), median_time(fwd_saved, 3), median_time(bwd, 3)
        mem_f, mem_fs, mem_b = peak_mem(fwd), peak_mem(fwd_saved), peak_mem(bwd)
        print(f"B={B}: 3x3 layers {fl / 1e9:.1f} GFLOP forward (direct-equivalent); backward = input gradients (same count) + "
              f"weight gradients (same count)")
        print(f"  no-grad forward        {t_f:8.3f} ms  {fl / t_f / 1e9:6.1f} TFLOP/s   peak memory {mem_f:8.1f} MiB")
        print(f"  forward, tensors saved {t_fs:8.3f} ms                     peak memory {mem_fs:8.1f} MiB")
        print(f"  backward               {t_b:8.3f} ms  {2 * fl / t_b / 1e9:6.1f} TFLOP/s   peak memory {mem_b:8.1f} MiB "
              f"(+ saved tensors)   backward / no-grad forward: {t_b / t_f:.2f}x")
        # the backward's parts, each layer alone on its own shapes
        tw, ti, classes = 0.0, 0.0, {}
        for c, ci, co, h, w in layer_shapes(B):
            up = 2 if c["pre"] == "up" else 1
            dZ = torch.randn(B, co, h, w, device=dev)
            X = torch.randn(B, ci, h // up, w // up, device=dev)
            tl = median_time(lambda: ops.cvn_wgrad(dZ, X, dil=c["dil"], in_up=up), 5)
            tw += tl
            cls = f"{ci}->{co} at {h}x{w} dil {c['dil']}" + (" in_up" if up == 2 else "")
            a = classes.setdefault(cls, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += tl
            a[2] += 2.0 * B * h * w * ci * co * 9
            if c["src"] != "x":
                key = c["key"]
                wt, packs = m._bwd_filters(key)
                ti += median_time(lambda: ops.conv3x3(dZ, wt, packs, None, dil=c["dil"], layer="cvn_bwd." + key), 5)
        print(f"  backward parts (each layer alone): weight gradients {tw:.3f} ms, input gradients {ti:.3f} ms, "
              f"rest (head, InstanceNorm, ReLU, d x of conv1_1.0) ~{max(t_b - tw - ti, 0):.3f} ms")
        for cls, (n, tl, f) in classes.items():
            print(f"    wgrad {cls:38s} x{n:2d}  {tl:7.3f} ms  {f / tl / 1e9:6.1f} TFLOP/s = {f / tl / 1e9 / (PEAK / 1e12):.2f} of "
                  f"fp32 MFMA peak")
        del saved, rstd, t


if __name__ == "__main__":
    main()
