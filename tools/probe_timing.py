"""What the backward probes (vgg_bwd_probe.py, cvn_bwd_probe.py, warp_bwd_probe.py) share: GPU time by HIP events with the launch
queue primed, its median / spread over rounds, and the peak device memory of a call.  Each probe passes its own round counts."""
import statistics

import torch

_filler = None


def device_time(fn, reps, warm=True):
    """ms per call with the launch queue primed (filler GEMMs enqueued first: the events bracket kernel execution only).
    warm: one untimed call first (a probe that has warmed every shape itself passes False)."""
    global _filler
    if _filler is None:
        _filler = (torch.randn(8192, 8192, device="cuda"), torch.randn(8192, 8192, device="cuda"),
                   torch.empty(8192, 8192, device="cuda"))
    if warm:
        fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2 + 4 * reps):
        torch.mm(_filler[0], _filler[1], out=_filler[2])
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def median_time(fn, reps, rounds):
    return statistics.median(device_time(fn, reps) for _ in range(rounds))


def spread(samples):
    """(p10, median, p90)"""
    s = sorted(samples)
    return s[max(0, int(0.1 * (len(s) - 1)))], statistics.median(s), s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))]


def peak_mem(fn):
    """MiB the call allocates on top of what is live before it (its result is kept alive until the device is idle)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    del keep
    return (torch.cuda.max_memory_allocated() - base) / 2**20
