"""What one optimiser step costs on the real parameter sets: dvc_amd.optim.Adam (one dvc_adam_step launch) and
dvc_amd.optim.CapturableAdam (dvc_adam_advance + dvc_adam_step on resident tables: eager with unchanged gradient addresses, and as a
replayed one-step graph followed by mark_updated()) beside torch.optim.Adam in its default mode, with foreach=True and with fused=True.  Per set: GPU time of the kernel alone (HIP events, launch queue primed,
launches on a resident table), GPU-side time of back-to-back step() calls (events; this is max(host, GPU) when the host is the
slower side), host time to issue a step (host clock around step() calls that end in one synchronise, queue drained first), and the
kernel's achieved bytes/s against the 28 B / element Adam has to move, as a fraction of the chip's measured HBM rate.

    python tools/adam_probe.py [--out profiles/adam_probe.txt]
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import probe_timing as T  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12          # bytes/s: float4 copy, and the data sheet
LR, BETAS = 2e-4, (0.5, 0.999)
ROUNDS, REPS = 7, 20


def parameter_sets():
    from dvc_amd.gan import Discriminator_x64
    from models.ColorVidNet import ColorVidNet
    from models.NonlocalNet import WarpNet
    with contextlib.redirect_stdout(io.StringIO()):
        col, warp, disc = ColorVidNet(7).cuda(), WarpNet(1).cuda(), Discriminator_x64(6, 64).cuda()
    col_p, warp_p = list(col.parameters()), list(warp.parameters())
    disc_p = [p for p in disc.parameters() if p.requires_grad]
    return [("ColorVidNet", [{"params": col_p}]), ("WarpNet", [{"params": warp_p}]), ("Discriminator_x64(6, 64)", [{"params": disc_p}]),
            ("generator (WarpNet at lr + ColorVidNet at 2 lr)", [{"params": warp_p, "lr": LR}, {"params": col_p, "lr": 2 * LR}])]


def host_issue_ms(step):
    samples = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            step()
        samples.append((time.perf_counter() - t0) * 1e3 / REPS)
        torch.cuda.synchronize()
    return T.spread(samples)


def kernel_only_ms(opt):
    """dvc_adam_step alone: the tables of a real step kept resident, launched back to back."""
    from dvc_amd import ops, optim
    real, kept = ops.adam_step, []

    def keep(tensor_table, n_tensors, chunk_table, n_chunks):
        kept.append((tensor_table.clone(), n_tensors, n_chunks))
        return real(tensor_table, n_tensors, chunk_table, n_chunks)

    ops.adam_step = keep
    try:
        opt.step()
    finally:
        ops.adam_step = real
    table, n_t, n_c = kept[0]
    chunks = table[n_t * optim.TENSOR_DTYPE.itemsize:]
    return T.spread([T.device_time(lambda: real(table, n_t, chunks, n_c), REPS) for _ in range(ROUNDS)]), n_c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_probe.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "adam_probe needs a GPU"
    from dvc_amd.optim import Adam, CapturableAdam
    lines = [f"Adam step on the real parameter sets, lr {LR}, betas {BETAS}, {torch.cuda.get_device_name(0)}; ms as p10 / median / p90 of "
             f"{ROUNDS} rounds x {REPS} steps"]
    for name, groups in parameter_sets():
        params = [p for g in groups for p in g["params"]]
        n = sum(p.numel() for p in params)
        gen = torch.Generator(device="cuda").manual_seed(0)
        for p in params:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
        lines.append(f"{name}: {len(params)} tensors, {n:,} elements ({min(p.numel() for p in params):,} .. {max(p.numel() for p in params):,}), "
                     f"{28 * n / 1e6:.1f} MB to move per step")
        makers = [("dvc_amd.optim.Adam", lambda gs: Adam(gs, lr=LR, betas=BETAS)),
                  ("CapturableAdam, eager", lambda gs: CapturableAdam(gs, lr=LR, betas=BETAS)),
                  ("torch default", lambda gs: torch.optim.Adam(gs, lr=LR, betas=BETAS)),
                  ("torch foreach=True", lambda gs: torch.optim.Adam(gs, lr=LR, betas=BETAS, foreach=True)),
                  ("torch fused=True", lambda gs: torch.optim.Adam(gs, lr=LR, betas=BETAS, fused=True))]
        medians = {}
        for label, make in makers:
            opt = make([dict(g) for g in groups])
            for _ in range(3):
                opt.step()
            torch.cuda.synchronize()
            gpu = T.spread([T.device_time(opt.step, REPS, warm=False) for _ in range(ROUNDS)])
            host = host_issue_ms(opt.step)
            medians[label] = (gpu[1], host[1])
            lines.append(f"  {label:<20s} back-to-back steps, GPU side {gpu[0]:.3f} / {gpu[1]:.3f} / {gpu[2]:.3f} ms   host issue "
                         f"{host[0]:.3f} / {host[1]:.3f} / {host[2]:.3f} ms")
            if label == "dvc_amd.optim.Adam":
                k, n_c = kernel_only_ms(opt)
                rate = 28 * n / (k[1] * 1e-3)
                lines.append(f"  {'dvc_adam_step alone':<20s} {k[0]:.4f} / {k[1]:.4f} / {k[2]:.4f} ms over {n_c:,} chunks = {rate / 1e12:.2f} TB/s of the 28 B / "
                             f"element = {100 * rate / HBM_MEASURED:.0f} % of the measured HBM rate (6.29 TB/s), {100 * rate / HBM_SPEC:.0f} % of the "
                             f"8.0 TB/s data sheet (resident p, g, m, v: {16 * n / 2**20:.0f} MiB against the 256 MiB Infinity Cache, "
                             f"which back-to-back launches on one table can hit)")
                medians["kernel"] = k[1]
            if label == "CapturableAdam, eager":           # the same optimiser, one step captured (gradient addresses unchanged)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()

                def replay():
                    graph.replay()
                    opt.mark_updated()

                replay()
                torch.cuda.synchronize()
                gpu = T.spread([T.device_time(replay, REPS, warm=False) for _ in range(ROUNDS)])
                host = host_issue_ms(replay)
                medians["CapturableAdam, replay"] = (gpu[1], host[1])
                lines.append(f"  {'CapturableAdam replay':<20s} replay + mark_updated, GPU side {gpu[0]:.3f} / {gpu[1]:.3f} / {gpu[2]:.3f} ms   host issue "
                             f"{host[0]:.3f} / {host[1]:.3f} / {host[2]:.3f} ms")
        ours, fused, default = medians["dvc_amd.optim.Adam"], medians["torch fused=True"], medians["torch default"]
        eager, replayed = medians["CapturableAdam, eager"], medians["CapturableAdam, replay"]
        lines.append(f"  host issue, CapturableAdam / Adam: eager {eager[1] / ours[1]:.2f}, replay {replayed[1] / ours[1]:.2f}   "
                     f"CapturableAdam / torch fused: eager {eager[1] / fused[1]:.2f}, replay {replayed[1] / fused[1]:.2f}   "
                     f"GPU side, CapturableAdam / torch fused: eager {eager[0] / fused[0]:.2f}, replay {replayed[0] / fused[0]:.2f}")
        lines.append(f"  GPU side, dvc / torch fused: {ours[0] / fused[0]:.2f}   host issue, dvc / torch default: {ours[1] / default[1]:.2f}   "
                     f"kernel alone / torch fused GPU side: {medians['kernel'] / fused[0]:.2f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
