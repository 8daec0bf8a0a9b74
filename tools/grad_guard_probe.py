"""What the gradient guard costs on the real parameter sets (those of tools/adam_probe.py): dvc_amd.optim.GuardedAdam (dvc_grad_norm's
two launches + dvc_adam_advance_guarded + dvc_adam_step_guarded on resident tables, clipping active) beside CapturableAdam (the
reference: its rows must reproduce profiles/adam_probe.txt within that file's run-to-run spread), each eagerly with unchanged
gradient addresses and as a replayed one-step graph followed by mark_updated(), and beside
torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.Adam(fused=True).  Per set: GPU-side time of back-to-back steps (HIP
events, launch queue primed), host time to issue a step, and dvc_grad_norm alone as bytes/s of the 4 B / element it reads.
Every variant is measured once per round, the rounds alternating in one process.

    python tools/grad_guard_probe.py [--out profiles/grad_guard_probe.txt]
"""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import probe_timing as T  # noqa: E402
from adam_probe import BETAS, HBM_MEASURED, LR, REPS, ROUNDS, parameter_sets  # noqa: E402

MAX_NORM = 1.0


def host_ms(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        step()
    ms = (time.perf_counter() - t0) * 1e3 / REPS
    torch.cuda.synchronize()
    return ms


def captured(opt):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()

    def replay():
        graph.replay()
        opt.mark_updated()

    return replay, graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard_probe.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "grad_guard_probe needs a GPU"
    from dvc_amd import ops, optim
    lines = [f"Guarded Adam step on the real parameter sets, lr {LR}, betas {BETAS}, max_grad_norm {MAX_NORM}, {torch.cuda.get_device_name(0)}; "
             f"ms as p10 / median / p90 of {ROUNDS} rounds x {REPS} steps, the variants alternating within a round"]
    for name, groups in parameter_sets():
        params = [p for g in groups for p in g["params"]]
        n = sum(p.numel() for p in params)
        gen = torch.Generator(device="cuda").manual_seed(0)
        for p in params:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
        lines.append(f"{name}: {len(params)} tensors, {n:,} elements, {28 * n / 1e6:.1f} MB for Adam to move per step + {4 * n / 1e6:.1f} MB for the norm to read")
        fresh = lambda: [dict(g) for g in groups]       # noqa: E731
        cap, cap_g = optim.CapturableAdam(fresh(), lr=LR, betas=BETAS), optim.CapturableAdam(fresh(), lr=LR, betas=BETAS)
        grd, grd_g = (optim.GuardedAdam(fresh(), lr=LR, betas=BETAS, max_grad_norm=MAX_NORM) for _ in range(2))
        fused = torch.optim.Adam(fresh(), lr=LR, betas=BETAS, fused=True)

        def torch_step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            fused.step()

        for opt in (cap, cap_g, grd, grd_g):
            for _ in range(3):
                opt.step()
        for _ in range(3):
            torch_step()
        torch.cuda.synchronize()
        cap_replay, g0 = captured(cap_g)
        grd_replay, g1 = captured(grd_g)
        res = grd._dvc_resident
        partials, guard = res.scratch.view(torch.float64), optim.new_guard(params[0].device)
        norm_alone = lambda: ops.grad_norm(res.table, res.n_t, res.chunks, res.n_c, partials, math.inf, guard)     # noqa: E731
        variants = [("CapturableAdam, eager", cap.step), ("CapturableAdam replay", cap_replay), ("GuardedAdam, eager", grd.step),
                    ("GuardedAdam replay", grd_replay), ("torch clip + fused", torch_step), ("dvc_grad_norm alone", norm_alone)]
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        gpu, host = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}
        for _ in range(ROUNDS):
            for label, fn in variants:
                gpu[label].append(T.device_time(fn, REPS, warm=False))
        for _ in range(ROUNDS):
            for label, fn in variants:
                host[label].append(host_ms(fn))
        med = {}
        for label, _ in variants:
            g, h = T.spread(gpu[label]), T.spread(host[label])
            med[label] = (g[1], h[1])
            lines.append(f"  {label:<22s} GPU side {g[0]:.4f} / {g[1]:.4f} / {g[2]:.4f} ms   host issue {h[0]:.3f} / {h[1]:.3f} / {h[2]:.3f} ms")
        k = med["dvc_grad_norm alone"][0]
        rate = 4 * n / (k * 1e-3)
        lines.append(f"  dvc_grad_norm alone over {res.n_c:,} chunks = {rate / 1e12:.2f} TB/s of the 4 B / element = {100 * rate / HBM_MEASURED:.0f} % of the "
                     f"measured HBM rate (6.29 TB/s); back-to-back launches re-read the same {4 * n / 2**20:.0f} MiB of gradients, which the 256 MiB "
                     f"Infinity Cache can hold")
        r = lambda a, b, i: med[a][i] / med[b][i]       # noqa: E731
        lines.append(f"  GPU side, GuardedAdam / CapturableAdam: eager {r('GuardedAdam, eager', 'CapturableAdam, eager', 0):.2f}, replay "
                     f"{r('GuardedAdam replay', 'CapturableAdam replay', 0):.2f}   GuardedAdam / torch clip + fused: eager "
                     f"{r('GuardedAdam, eager', 'torch clip + fused', 0):.2f}, replay {r('GuardedAdam replay', 'torch clip + fused', 0):.2f}")
        lines.append(f"  host issue, GuardedAdam / CapturableAdam: eager {r('GuardedAdam, eager', 'CapturableAdam, eager', 1):.2f}, replay "
                     f"{r('GuardedAdam replay', 'CapturableAdam replay', 1):.2f}   GuardedAdam / torch clip + fused: eager "
                     f"{r('GuardedAdam, eager', 'torch clip + fused', 1):.2f}, replay {r('GuardedAdam replay', 'torch clip + fused', 1):.2f}")
        skipped = int(grd.skipped_steps.item()) + int(grd_g.skipped_steps.item())
        lines.append(f"  skipped steps during the run: {skipped}   last norm {grd.last_grad_norm.item():.4g}")
        del g0, g1
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
