#!/usr/bin/env python
"""Which C-ABI calls does the Python side make, with which arguments, and what comes out?

Wraps every `dvc_*` entry point of the loaded library and logs, per call, the function name, every scalar argument, the fields
of every descriptor / item structure, and for every pointer whether it is NULL — no addresses, so two runs of the same code
give the same log.  Runs one frame of the clip driver, one training step of ColorVidNet, one of WarpNet's trunk and one VGG19
forward + input gradient at 216x384, first under the defaults and then with each launch-deciding switch flipped once, and
writes
    <out>.calls.txt     one line per call
    <out>.digests.txt   SHA-256 (16 hex digits) of the raw bytes of every result tensor
A change that must not alter what is launched (a refactor of dvc_amd/ops.py) is checked by running this file against the
two trees and comparing the two pairs of files line for line.

    python tools/launch_log.py OUT_PREFIX [--tree PATH_TO_ANOTHER_CHECKOUT] [--autotune-cache FILE.json] [--prime]

--tree: import the package from another checkout (the commit to compare against, exported by the caller with `git worktree`
or `git archive`; it is not part of this repository and nothing here depends on it).
--autotune-cache: the autotuner picks by timing, so two runs of the SAME code log different configurations; with a persisted
table (DVC_AUTOTUNE_CACHE) it replays choices instead.  `--prime` runs the workloads once with the autotuner on, only to write
that table; later runs given the same file add the configuration `autotune=1` and replay it, launch for launch.
"""
import contextlib
import ctypes
import hashlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
TUNE_CACHE = os.path.abspath(sys.argv[sys.argv.index("--autotune-cache") + 1]) if "--autotune-cache" in sys.argv else None
if TUNE_CACHE:
    os.environ["DVC_AUTOTUNE_CACHE"] = TUNE_CACHE        # (read when dvc_amd.ops is imported)
for p in (os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd"), ROOT):
    sys.path.insert(0, p)
import torch  # noqa: E402

from dvc_amd import _lib, ops, synth  # noqa: E402
from dvc_amd.frame import ClipColorizer  # noqa: E402
from models.ColorVidNet import ColorVidNet  # noqa: E402
from models.NonlocalNet import VGG19_pytorch, WarpNet  # noqa: E402

H, W = 216, 384
calls, digests = [], []


def _show(v, ctype=None):
    """One argument as text: pointers as NULL / ptr, structures field by field, everything else by value."""
    if v is None:
        return "NULL"
    if isinstance(v, ctypes.c_void_p):
        return "ptr" if v.value else "NULL"
    if isinstance(v, ctypes.Array) and isinstance(v[0], ctypes.Structure):
        return "[" + ", ".join(_show(e) for e in v) + "]"
    if ctype is ctypes.c_void_p:
        return "ptr" if (v if isinstance(v, int) else ctypes.cast(v, ctypes.c_void_p).value) else "NULL"
    if hasattr(v, "_obj"):                  # ctypes.byref(...)
        return _show(v._obj)
    if isinstance(v, ctypes.Structure):
        return "{" + " ".join(f"{f}={_show(getattr(v, f), t)}" for f, t in v._fields_) + "}"
    if isinstance(v, ctypes._SimpleCData):
        return "out" if isinstance(v, ctypes.c_int32) else repr(v.value)
    return repr(v)


class LoggingLib:
    """The loaded library with every dvc_* call logged to `calls` before it is forwarded."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dvc_") or name in ("dvc_last_error", "dvc_abi_version"):
            return fn
        argtypes = _lib.SIGNATURES[name][1]

        def logged(*args):
            calls.append(name + "(" + ", ".join(_show(a, t) for a, t in zip(args, argtypes)) + ")")
            return fn(*args)
        return logged


def digest(label, t):
    if t is None:
        digests.append(f"{'-' * 16}  {label}")
        return
    digests.append(hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16] + "  " + label)


_sd = []


def build():
    if not _sd:
        _sd.extend((synth.vgg19_state_dict(0), synth.warpnet_state_dict(0), synth.colorvidnet_state_dict(0, contractive=True)))
    with contextlib.redirect_stdout(io.StringIO()):
        vgg, warp, cvn = VGG19_pytorch(), WarpNet(1), ColorVidNet(7)
    for m, sd in zip((vgg, warp, cvn), _sd):
        m.load_state_dict(sd)
    for m in (vgg, warp, cvn):
        m.cuda()
    return vgg, warp, cvn


def run_all(tag):
    """The four workloads from fresh modules (so that every weight is packed under the switches in force)."""
    calls.append(f"==== {tag}")
    vgg, warp, cvn = build()
    g = torch.Generator().manual_seed(0)
    # one frame of the clip driver (and the per-frame API next to it)
    for m in (vgg, warp, cvn):
        m.eval()
    cc = ClipColorizer(vgg, warp, cvn)
    cc.set_exemplar(synth.synth_lab(2, H, W).cuda())
    fr = [synth.synth_lab(1000 + i, H, W).cuda() for i in range(2)]
    calls.append("-- frame")
    ab, _ = cc.frame(fr[0], torch.zeros_like(fr[0]))
    digest(f"{tag} frame ab", ab)
    calls.append("-- clip")
    for i, o in enumerate(cc.clip(fr, lookahead=1)):
        digest(f"{tag} clip ab {i}", o)
    # one training step of ColorVidNet
    calls.append("-- cvn step")
    cvn.train()
    x = (torch.rand(2, 7, H, W, generator=g) * 100 - 50).cuda().requires_grad_(True)
    gab = torch.randn(2, 2, H, W, generator=g).cuda()
    out = cvn(x)
    out.backward(gab)
    digest(f"{tag} cvn out", out)
    for n, p in cvn.named_parameters():
        digest(f"{tag} cvn grad {n}", p.grad)
    digest(f"{tag} cvn dx", x.grad)
    # one training step of WarpNet's trunk
    calls.append("-- warp step")
    warp2 = build()[1]
    for name in ("layer2_1", "layer3_1", "layer4_1", "layer5_1"):
        for p in getattr(warp2, name).parameters():
            p.requires_grad = False
    warp2.train()
    h, w = H // 4, W // 4
    tA = (torch.randn(2, 256, h, w, generator=g).abs() * 0.5).cuda().requires_grad_(True)
    tB = (torch.randn(2, 256, h, w, generator=g).abs() * 0.5).cuda().requires_grad_(True)
    blab = (torch.randn(2, 3, h, w, generator=g) * 30).cuda()
    gy, gs = torch.randn(2, 3, H, W, generator=g).cuda(), torch.randn(2, 1, H, W, generator=g).cuda()
    names, params = zip(*warp2._trunk_named_parameters())
    y, sim = warp2._train_from_trunks(tA, tB, blab, 0.01)
    grads = torch.autograd.grad((y * gy).sum() + (sim * gs).sum(), list(params) + [tA, tB])
    digest(f"{tag} warp y", y)
    digest(f"{tag} warp similarity_map", sim)
    for n, gr in zip(list(names) + ["seam dA", "seam dB"], grads):
        digest(f"{tag} warp grad {n}", gr)
    # VGG19 forward + input gradient
    calls.append("-- vgg backward")
    for p in vgg.parameters():
        p.requires_grad = False
    keys = ["r12", "r22", "r32", "r42", "r52"]
    xv = torch.rand(2, 3, H, W, generator=g).cuda().requires_grad_(True)
    outs = vgg(xv, keys)
    torch.autograd.backward(outs, [torch.randn(o.shape, generator=g).cuda() for o in outs])
    for k, o in zip(keys, outs):
        digest(f"{tag} vgg {k}", o)
    digest(f"{tag} vgg dx", xv.grad)
    torch.cuda.synchronize()


# every launch-deciding switch, flipped once through its public setter: (tag, flip, restore); batch_plan is a context manager
# (main), and the autotuner runs from a persisted table only (--autotune-cache).
FLIPS = [
    ("conv_algo=direct", lambda: ops.set_conv_algo("direct"), lambda: ops.set_conv_algo("auto")),
    ("conv_algo=speed", lambda: ops.set_conv_algo("speed"), lambda: ops.set_conv_algo("auto")),
    ("fuse_reduce=0", lambda: ops.set_fuse_reduce(False), lambda: ops.set_fuse_reduce(True)),
    ("pool_fusion=0", lambda: ops.set_pool_fusion(False), lambda: ops.set_pool_fusion(True)),
    ("dual_conv=0", lambda: ops.set_dual_conv(False), lambda: ops.set_dual_conv(True)),
    ("fold_merge=0", lambda: ops.set_fold_merge(False), lambda: ops.set_fold_merge(True)),
    ("direct_layers=vgg.conv3_1", lambda: ops.set_direct_layers(["vgg.conv3_1"]), lambda: ops.set_direct_layers(None)),
    ("group_heads=0", lambda: ops.set_group_heads(False), lambda: ops.set_group_heads(True)),
    ("ws_conv=0", lambda: ops.set_ws_conv(False), lambda: ops.set_ws_conv(True)),
    ("gray_fusion=0", lambda: ops.set_gray_fusion(False), lambda: ops.set_gray_fusion(True)),
]


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    out = sys.argv[1]
    _lib._lib = LoggingLib(_lib.load())
    if "--prime" in sys.argv:
        assert TUNE_CACHE, "--prime needs --autotune-cache"
        ops.set_autotune(True)
        run_all("prime")
        print(f"{TUNE_CACHE}: {len(ops.autotune_table())} tuned geometries")
        return
    run_all("defaults")
    with ops.batch_plan(True):
        run_all("batch_plan=1")
    for tag, flip, restore in FLIPS:
        flip()
        try:
            run_all(tag)
        finally:
            restore()
    if TUNE_CACHE:
        ops.set_autotune(True)          # loads the table
        known = len(ops.autotune_table())
        assert known, f"{TUNE_CACHE} holds no table: run with --prime first"
        try:
            run_all("autotune=1")
        finally:
            ops.set_autotune(False)
        assert len(ops.autotune_table()) == known, "a geometry was missing from the persisted table and was tuned by timing"
    for path, lines in ((out + ".calls.txt", calls), (out + ".digests.txt", digests)):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{path}: {len(lines)} lines, sha256 {hashlib.sha256(open(path, 'rb').read()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
