"""What the whole loss stage of one step costs with a resident plan, at tools/loss_probe.py's size and term set (batch 16, 216 x 384:
three terms on the predicted ab, the perceptual MSE on relu5_2) plus the two relativistic GAN terms on a discriminator output of
the shape Discriminator_x64(6, 64) returns there, [16, 1].  Forward + backward, four ways ALTERNATED inside every round of one run:

    plan, eager hit     dvc_amd.losses.Plan called eagerly with no input moved (how many calls still uploaded a table is reported)
    plan, replayed      the same call and its backward captured once, replayed from the graph
    fused + torch GAN   the parent's way: losses.fused for the four pixel terms, the GAN terms as torch expressions
    torch composition   every term as the reference's torch expression

GPU time by HIP events with the launch queue primed (tools/probe_timing.py: device_time) and host issue time (the wall clock of
issuing the calls, device idle before and not waited for), p10 / median / p90 over the rounds.

    python tools/loss_plan_probe.py [--out profiles/loss_plan_probe.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import probe_timing as T  # noqa: E402
from loss_probe import B, make_terms  # noqa: E402

ROUNDS, REPS = 11, 10
W_GAN = 0.2


def host_time(fn, reps):
    """ms of host time per call to ISSUE fn: the device is idle at the start and is not waited for inside the bracket."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_plan_probe.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_plan_probe needs a GPU"
    from dvc_amd import losses
    pixel, leaves = make_terms()
    g = torch.Generator(device="cuda").manual_seed(1)
    y_fake = torch.randn(B, 1, device="cuda", generator=g).requires_grad_(True)
    y_real = torch.randn(B, 1, device="cuda", generator=g).requires_grad_(True)
    leaves = tuple(leaves) + (y_fake, y_real)
    gan = [("rel", y_fake, y_real, -1.0, 0.5 * W_GAN), ("rel", y_real, y_fake, 1.0, 0.5 * W_GAN)]
    terms = pixel + gan
    plan = losses.Plan()

    def clear():
        for v in leaves:
            v.grad = None

    def torch_gan():
        return 0.5 * W_GAN * (torch.mean((y_fake - torch.mean(y_real) + 1) ** 2) + torch.mean((y_real - torch.mean(y_fake) - 1) ** 2))

    def run_plan():
        clear()
        plan(terms)[0].backward()

    def run_parent():
        clear()
        (losses.fused(pixel)[0] + torch_gan()).backward()

    def run_torch():
        clear()
        total = torch_gan()
        for kind, x, t, w, s in pixel:
            out = (x - t) ** 2 if kind == "mse" else torch.abs(x - t)
            if w is not None:
                out = out * w.expand_as(out)
            total = total + s * out.mean()
        total.backward()

    for _ in range(4):          # tables, spares, and the gradients' addresses settle
        run_plan()
    want = plan(terms)[0].detach().clone()
    ref = (losses.fused(pixel)[0] + torch_gan()).detach()
    assert abs(want.item() - ref.item()) <= 1e-5 * abs(ref.item()), (want.item(), ref.item())
    # the same call captured: a plan and leaves of its own; the eager call that comes first runs on the stream the capture will
    # use, so a gradient accumulator that outlives it belongs to that stream and the captured backward stays one straight line
    cap, side = losses.Plan(), torch.cuda.Stream()
    twin = {id(v): v.detach().clone().requires_grad_(True) for v in leaves}
    cap_terms = [(k, twin.get(id(a), a), twin.get(id(b), b) if isinstance(b, torch.Tensor) else b, c, s) for k, a, b, c, s in terms]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap(cap_terms)[0].backward()
    for v in twin.values():
        v.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        total, _ = cap(cap_terms)
        total.backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(total.detach(), want), (total.item(), want.item())

    runs = (("plan, eager hit", run_plan), ("plan, replayed", graph.replay), ("fused + torch GAN", run_parent),
            ("torch composition", run_torch))
    gpu, host = {k: [] for k, _ in runs}, {k: [] for k, _ in runs}
    for _, fn in runs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    uploads = plan.uploads
    for _ in range(ROUNDS):
        for label, fn in runs:          # alternated inside the round: drift hits every variant alike
            gpu[label].append(T.device_time(fn, REPS, warm=False))
            host[label].append(host_time(fn, REPS))
    calls, misses = 2 * ROUNDS * REPS, plan.uploads - uploads       # (the inputs never move: a miss is the backward's, whose
    # gradients the allocator placed elsewhere after another variant's turn)
    lines = [f"Loss stage of one step, batch {B} at 216x384, {torch.cuda.get_device_name(0)}: tools/loss_probe.py's four pixel terms + two "
             f"relativistic GAN terms on [16,1]; forward + backward; ms as p10 / median / p90 of {ROUNDS} rounds x {REPS} repeats, the four "
             f"variants alternated inside every round; of the {calls} measured eager plan calls {misses} uploaded a table (the backward's), the others were fingerprint hits in both directions"]
    for label, _ in runs:
        a, b = T.spread(gpu[label]), T.spread(host[label])
        lines.append(f"  {label:<20s} GPU {a[0]:.4f} / {a[1]:.4f} / {a[2]:.4f}   host issue {b[0]:.4f} / {b[1]:.4f} / {b[2]:.4f}")
    med = {k: T.spread(v)[1] for k, v in host.items()}
    lines.append(f"  host issue, plan eager hit / torch composition: {med['plan, eager hit'] / med['torch composition']:.2f}   "
                 f"plan eager hit / fused + torch GAN: {med['plan, eager hit'] / med['fused + torch GAN']:.2f}")
    lines.append("  (not measured: a whole training iteration in one graph)")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
