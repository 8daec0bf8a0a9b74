"""What the pixel losses of one generator step cost at train.py's size (216 x 384, batch 16): three terms on the predicted ab
[16,2,216,384] — L1 to the ground truth, MSE to a weighted-average output, MSE to the warped previous prediction under the
[16,1,216,384] occlusion mask — and the perceptual MSE on relu5_2 features [16,512,13,24].  Forward + backward (the gradient to the
prediction / the predicted features), three ways in one run: ONE dvc_amd.losses.fused call, FOUR helper calls, and the torch
composition of the reference's expressions.  GPU time by HIP events with the launch queue primed (tools/probe_timing.py:
device_time, the method of tools/training_side_probe.py), p10 / median / p90 over back-to-back rounds, and the bytes the terms have
to move per second.  The library's launches are also timed alone on resident tables (no staging copy, no torch allocation).

    python tools/loss_probe.py [--out profiles/loss_probe.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import probe_timing as T  # noqa: E402

HBM_MEASURED = 6.29e12          # bytes/s: float4 copy (tools/adam_probe.py)
ROUNDS, REPS = 9, 10
B, H, W = 16, 216, 384


def make_terms():
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)     # noqa: E731
    ab = r(B, 2, H, W).requires_grad_(True)
    mask = (torch.rand(B, 1, H, W, device="cuda", generator=g) < 0.8).float()
    feat = r(B, 512, 13, 24).requires_grad_(True)
    terms = [("l1", ab, r(B, 2, H, W), None, 2.0), ("mse", ab, r(B, 2, H, W), None, 5.0), ("mse", ab, r(B, 2, H, W), mask, 0.02),
             ("mse", feat, r(B, 512, 13, 24), None, 0.001)]
    return terms, (ab, feat)


def bytes_moved(terms):
    """Forward reads x, t (and w); backward reads them again and writes dx."""
    total = 0
    for _, x, t, w, _ in terms:
        total += 4 * (2 * (2 * x.numel() + (0 if w is None else w.numel())) + x.numel())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_probe.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_probe needs a GPU"
    from dvc_amd import losses, ops
    terms, leaves = make_terms()
    helper = {("l1", False): losses.l1_loss, ("mse", False): losses.mse_loss, ("l1", True): losses.weighted_l1_loss,
              ("mse", True): losses.weighted_mse_loss}

    def clear():
        for v in leaves:
            v.grad = None

    def run_fused():
        clear()
        losses.fused(terms)[0].backward()

    def run_helpers():
        clear()
        total = 0
        for kind, x, t, w, s in terms:
            v = helper[kind, w is not None](x, t) if w is None else helper[kind, True](x, t, w)
            total = total + s * v
        total.backward()

    def run_torch():
        clear()
        total = 0
        for kind, x, t, w, s in terms:
            out = (x - t) ** 2 if kind == "mse" else torch.abs(x - t)
            if w is not None:
                out = out * w.expand_as(out)
            total = total + s * out.mean()
        total.backward()

    # the library's launches alone, on resident tables with gradient buffers of their own
    import numpy as np
    dxs = [torch.empty_like(x) for _, x, _, _, _ in terms]
    entries = []
    for (kind, x, t, w, s), dx in zip(terms, dxs):
        plane, cpl = (x.shape[2] * x.shape[3], x.shape[1] * x.shape[2] * x.shape[3]) if w is not None and w.shape != x.shape else (1, 0)
        entries.append((x.data_ptr(), t.data_ptr(), 0 if w is None else w.data_ptr(), dx.data_ptr(), 0, x.numel(), plane, cpl,
                        losses.KINDS[kind], 0.0, s))
    term_np, chunk_np = losses.build_tables(entries)
    host = torch.from_numpy(np.concatenate([term_np.view(np.uint8), chunk_np.view(np.uint8)]))
    table, n, n_c = host.cuda(), len(term_np), len(chunk_np)
    chunks = table[term_np.nbytes:]
    partials = torch.empty(n_c, dtype=torch.float64, device="cuda")
    values, g_total = torch.empty(n + 1, device="cuda"), torch.ones(1, device="cuda")

    def run_kernels():
        ops.loss_fwd(table, host, n, chunks, n_c, partials, values)
        ops.loss_bwd(table, host, n, chunks, n_c, g_total)

    run_kernels()
    assert torch.equal(values[n], losses.fused(terms)[0].detach())      # the same tables as a real call's
    nbytes = bytes_moved(terms)
    lines = [f"Pixel losses of one generator step, batch {B} at {H}x{W}, {torch.cuda.get_device_name(0)}: ab [16,2,216,384] x 3 terms (one "
             f"masked by [16,1,216,384]) + relu5_2 [16,512,13,24] x 1; forward + backward, {nbytes / 1e6:.1f} MB to move "
             f"(x, t, w read twice, dx written); GPU ms as p10 / median / p90 of {ROUNDS} rounds x {REPS} back-to-back repeats, queue primed"]
    med = {}
    for label, fn in (("losses.fused, one call", run_fused), ("four helper calls", run_helpers), ("torch composition", run_torch),
                      ("dvc_loss_fwd + dvc_loss_bwd alone", run_kernels)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        s = T.spread([T.device_time(fn, REPS, warm=False) for _ in range(ROUNDS)])
        med[label] = s[1]
        rate = nbytes / (s[1] * 1e-3)
        lines.append(f"  {label:<36s} {s[0]:.4f} / {s[1]:.4f} / {s[2]:.4f} ms   {rate / 1e12:.2f} TB/s of the terms' own bytes "
                     f"({100 * rate / HBM_MEASURED:.0f} % of the measured 6.29 TB/s HBM rate)")
    lines.append(f"  (the torch composition moves more than the terms' own bytes: it writes and re-reads every intermediate; the resident "
                 f"working set, {nbytes / 2 / 2**20:.0f} MiB, fits the 256 MiB Infinity Cache, which back-to-back repeats can hit)")
    lines.append(f"  fused / torch: {med['losses.fused, one call'] / med['torch composition']:.2f}   helpers / torch: "
                 f"{med['four helper calls'] / med['torch composition']:.2f}   fused / helpers: "
                 f"{med['losses.fused, one call'] / med['four helper calls']:.2f}   launches alone / fused call: "
                 f"{med['dvc_loss_fwd + dvc_loss_bwd alone'] / med['losses.fused, one call']:.2f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
