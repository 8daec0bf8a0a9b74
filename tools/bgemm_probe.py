"""The training side's three row-block products on the four backends of dvc_amd.block_products — "split3" (csrc/bgemm_split3.hip:
three bf16 terms per operand on the bf16 MFMA), "native" (csrc/bgemm.hip through ops.bgemm), "vendor" (torch.bmm) and "engine"
(the 1x1-convolution engine) — at the production shape of the fused correlation's
backward: C = 256, P = 54 x 96 = 5184 positions, row blocks of R = 2048, one image and the 16 images that BLOCK_BYTES allows per
slice at batch 16.  Each product is issued alone, exactly as block_products issues it (the engine's staging copies and the
staged copy of a partial grad_rows included), then the whole backward passes of fused_correlation and ContextualLoss.

GPU time by HIP events with the launch queue primed (tools/probe_timing.py); the backends alternate inside every round, all in
one process; median and p10..p90 over the rounds.  TFLOP/s = 2 nb R P C / median (the fp32 product's operations, whatever
the backend spends on them); the share is of the 157.3 TFLOP/s fp32 matrix peak of the MI355X, and for split3 of an eighth of the
2500 TFLOP/s dense bf16 peak (eight bf16 products per fp32 product: 312.5 TFLOP/s).  The table goes to stdout and to --out (default profiles/bgemm_probe.txt).

    python tools/bgemm_probe.py [--out FILE] [--rounds N] [--trace]

--trace: one untimed pass over the native products only, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/bgemm_probe.py --trace)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from dvc_amd import block_products as bp, contextual, corr_autograd, ops  # noqa: E402
from probe_timing import device_time, spread  # noqa: E402

PEAK = 157.3
PEAKS = {"split3": 2500.0 / 8}                    # the others: PEAK
BACKENDS = ("split3", "native", "vendor", "engine")
C, H, W, R = 256, 54, 96, 2048
P = H * W


def product_calls(name, nb, gen):
    """The three products of one row block of `nb` images on backend `name`, as closures over a set-up block."""
    with bp.use_backend(name):
        L = torch.randn(nb, C, P, generator=gen, device="cuda")
        M = torch.randn(nb, C, P, generator=gen, device="cuda")
        prod = bp.block_products(L, M, (H, W), R, nb, want_rows=True, want_cols=True)
    assert prod.chunk == nb
    prod.images(slice(0, nb))
    prod.scores(0, R)
    for t in prod.ds_targets():
        if t is not None:
            t.normal_(generator=gen)
    d_cols, d_rows = torch.zeros_like(M), torch.zeros_like(L)
    return {"scores       S = L_blk^T M": lambda: prod.scores(0, R),
            "grad_cols    dM += L_blk dS": lambda: prod.grad_cols_accumulate(d_cols),
            "grad_rows    dL_blk = M dS^T": lambda: prod.grad_rows(d_rows)}


def backward_calls(gen):
    """Backward passes alone (the graph is retained; the leaf's .grad accumulation is part of the call)."""
    calls = {}
    for B in (1, 16):
        th = torch.randn(B, C, P, generator=gen, device="cuda")
        ph = torch.randn(B, C, P, generator=gen, device="cuda")
        th, ph = (t - t.mean(-1, keepdim=True) for t in (th, ph))
        th, ph = (t / t.norm(dim=1, keepdim=True) for t in (th, ph))
        blab = torch.randn(B, 3, P, generator=gen, device="cuda") * 30
        gy = torch.randn(B, 3, H, W, generator=gen, device="cuda")

        def corr(th=th, ph=ph, blab=blab, gy=gy):
            a, b = th.clone().requires_grad_(True), ph.clone().requires_grad_(True)
            y, _, _ = corr_autograd.fused_correlation(a, b, blab, 0.01, H, W)
            loss = (y * gy).sum()
            return lambda: loss.backward(retain_graph=True)
        calls[f"fused_correlation backward  B={B} 54x96"] = corr
    for (Cx, Hx, Wx, B) in ((512, 27, 48, 16), (512, 13, 24, 16)):
        X = torch.randn(B, Cx, Hx, Wx, generator=gen, device="cuda")
        Y = torch.randn(B, Cx, Hx, Wx, generator=gen, device="cuda")

        def cx(X=X, Y=Y):
            x = X.clone().requires_grad_(True)
            loss = contextual.ContextualLoss()(x, Y).sum()
            return lambda: loss.backward(retain_graph=True)
        calls[f"ContextualLoss backward     B={B} C={Cx} {Hx}x{Wx}"] = cx
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgemm_probe.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bgemm_probe needs a GPU"
    gen = torch.Generator(device="cuda").manual_seed(0)
    if args.trace:
        for nb in (1, 16):
            for fn in product_calls("native", nb, gen).values():
                fn()
        torch.cuda.synchronize()
        return
    lines = [f"torch {torch.__version__}; {torch.cuda.get_device_name(0)}; C={C} P={H}x{W}={P} R={R}; {args.rounds} rounds, "
             f"backends alternating; ms = median (p10..p90); TF = TFLOP/s at the median; share of {PEAK} TFLOP/s fp32 matrix peak "
             f"(split3: of {PEAKS['split3']:.1f} = the dense bf16 peak / 8)"]

    def run(title, per_backend, flops, reps):
        """per_backend: {backend: callable}; one line per backend."""
        samples = {n: [] for n in per_backend}
        for fn in per_backend.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for n, fn in per_backend.items():
                samples[n].append(device_time(fn, reps, warm=False))
        lines.append(title)
        med = {}
        for n, s in samples.items():
            lo, m, hi = spread(s)
            med[n] = m
            rate = f"  {flops / m / 1e9:6.1f} TF  {100 * flops / m / 1e9 / PEAKS.get(n, PEAK):5.1f} %" if flops else ""
            lines.append(f"    {n:7s} {m:9.3f} ms ({lo:.3f}..{hi:.3f}){rate}")
        lines.append("    native / vendor = %.2f, native / engine = %.2f" % (med["native"] / med["vendor"], med["native"] / med["engine"]))
        lines.append("    split3 / native = %.2f, split3 / vendor = %.2f" % (med["split3"] / med["native"], med["split3"] / med["vendor"]))
        print("\n".join(lines[-(len(per_backend) + 3):]), flush=True)

    print(lines[0], flush=True)
    for nb in (1, 16):
        calls = {n: product_calls(n, nb, gen) for n in BACKENDS}
        for label in calls["native"]:
            run(f"{label}   nb={nb}", {n: calls[n][label] for n in BACKENDS}, 2.0 * nb * R * P * C, 20 if nb == 1 else 5)
        del calls
        torch.cuda.empty_cache()
    whole = {}
    for n in BACKENDS:
        with bp.use_backend(n):
            whole[n] = {label: make() for label, make in backward_calls(gen).items()}
    for label in whole["native"]:
        def under(n, fn):
            def call():
                with bp.use_backend(n):
                    fn()
            return call
        run(label, {n: under(n, whole[n][label]) for n in BACKENDS}, 0.0, 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
