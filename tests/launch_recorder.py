"""The launch sequences of the three layer walks, recorded on the CPU (tests/test_arch_graph.py).

ColorVidNet._forward / _backward, WarpNet._heads and VGG19_pytorch._forward / _input_grad reach the device only through
`dvc_amd.ops`.  `record_all` swaps the entry points they call for stand-ins that return zero CPU tensors of the right shape and
log one record per call: the op, every argument by name — a tensor as its shape and the number of the buffer it lives in (buffers
are numbered as the sequence first meets them, so the record also says WHICH earlier result or parameter a launch reads), a
`packs` callable as a placeholder, everything else as it is.  The records say nothing about values: what they pin is which
launches a walk makes, in which order, on which tensors, with which keywords.

`python tests/launch_recorder.py OUT.json` writes the records; tests/golden/cvn_launch_sequence.json is that output at the
commit named in the file's "_commit" entry.
"""
import contextlib
import inspect
import io
import json
import os
import sys

import torch

ALL_VGG_TAPS = ["r12", "r22", "r32", "r42", "r52"]


def _standins(mp, ops, *, winograd=True, dual=True, pool_fusion=True):
    """Patch `ops` through the pytest MonkeyPatch `mp`; returns the list the records go to."""
    log, bufs, keep = [], {}, []

    def desc(v):
        if isinstance(v, torch.Tensor):
            ptr = v.untyped_storage().data_ptr()
            if ptr not in bufs:
                bufs[ptr] = len(bufs)
                keep.append(v)          # (alive to the end of the run: no address is handed out twice)
            d = {"shape": list(v.shape), "buf": bufs[ptr]}
            if v.storage_offset():
                d["offset"] = v.storage_offset()
            return d
        if isinstance(v, dict):
            return {k: desc(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [desc(x) for x in v]
        return "<callable>" if callable(v) else v

    def launch(fn):
        sig = inspect.signature(fn)

        def logged(*a, **kw):
            log.append({"op": fn.__name__, "args": desc(dict(sig.bind(*a, **kw).arguments))})
            return fn(*a, **kw)
        mp.setattr(ops, fn.__name__, logged)
        return fn

    def conv_out(x, cout, **geometry):
        return torch.zeros(x.shape[0], cout, *ops.conv_out_hw(x.shape[2], x.shape[3], **geometry))

    @launch
    def conv3x3(x, weight, packs, bias, *, dil=1, in_up=1, in_sub=1, out=None, **kw):
        return out if out is not None else conv_out(x, weight.shape[0], dil=dil, pad=dil, in_up=in_up, in_sub=in_sub)

    @launch
    def conv3x3_group(items):
        return [conv3x3(**it) for it in items]

    @launch
    def conv2d(x, w_packed, bias, *, ksize=3, stride=1, dil=1, pad=1, in_up=1, in_sub=1, out=None, **kw):
        return out if out is not None else conv_out(x, w_packed.shape[-1], ksize=ksize, stride=stride, dil=dil, pad=pad,
                                                    in_up=in_up, in_sub=in_sub)

    @launch
    def conv2d_winograd_dual(xA, xB, u_cat, bias, *, dil=1, in_upA=1, **kw):
        return conv_out(xA, u_cat.shape[0] * 32, dil=dil, pad=dil, in_up=in_upA)

    @launch
    def conv2d_winograd_pool(x, u_packed, bias, *, want_full=True, **kw):
        N, _, H, W = x.shape
        C = u_packed.shape[0] * 32
        return torch.zeros(N, C, H, W) if want_full else None, torch.zeros(N, C, H // 2, W // 2)

    @launch
    def conv1x1_small(x, w, bias, act=0):
        return torch.zeros(x.shape[0], w.shape[0], *x.shape[2:])

    @launch
    def instnorm_apply(x, *, up=1, sub=1, rpad=0, out=None, second=None, **kw):
        N, C, H, W = x.shape
        half = (N, C, (H + 1) // 2, (W + 1) // 2)
        if out is None:
            out = torch.zeros(half) if sub == 2 else torch.zeros(N, C, H * up + 2 * rpad, W * up)
        return out if second is None else (out, torch.zeros(half if second[1] == 2 else (N, C, H, W)))

    @launch
    def instnorm_apply_group(items):
        return [instnorm_apply(**it) for it in items]

    @launch
    def maxpool2x2(x):
        return torch.zeros(x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2)

    @launch
    def avgpool2x2(x):
        return maxpool2x2(x)

    @launch
    def cvn_head_bwd(ab, grad_ab, w_ab, R, slope=0.2):
        return torch.zeros_like(R), torch.zeros(2, R.shape[1], 1, 1), torch.zeros(2)

    @launch
    def cvn_wgrad(dZ, X, *, dil=1, in_up=1, splits=None):
        return torch.zeros(dZ.shape[1], X.shape[1], 3, 3), torch.zeros(dZ.shape[1])

    @launch
    def cvn_inorm_bwd(n, rstd, R, g_full=None, g_ss=None, ss_w=None, g_up=None):
        return torch.zeros_like(R), None if g_ss is None else torch.zeros(R.shape[1])

    @launch
    def vgg_act_bwd(dX, g, R, out=None):
        return out if out is not None else torch.zeros_like(R)

    @launch
    def vgg_pool_act_bwd(dP, gP, gR, R, avg=False):
        return torch.zeros_like(R)

    @launch
    def vgg_conv1_bwd(dZ, w_t):
        return torch.zeros(dZ.shape[0], 3, *dZ.shape[2:])

    # what selects launches, and the one pack the walks themselves ask the library for (cold path: not a record)
    def winograd_selected(N, Cin, H, W, Cout, *, ksize=3, stride=1, dil=1, pad=1, in_affine=False, in_prelu=False, **kw):
        return winograd and ops.winograd_eligible(Cin, Cout, ksize, stride, dil, pad, in_affine, in_prelu)

    mp.setattr(ops, "winograd_selected", winograd_selected)
    mp.setattr(ops, "dual_conv_enabled", lambda: dual)
    mp.setattr(ops, "pool_fusion", lambda: pool_fusion)
    mp.setattr(ops, "pack_winograd_weight", lambda w: torch.zeros(w.shape[0] // 32, w.shape[1], 4, 32, 4))
    return log


def _vgg_features(H, W):
    """Shapes of relu2_1 .. relu5_1 of an H x W frame (four floor-halving pools)."""
    out = []
    for c in (128, 256, 512, 512):
        H, W = H // 2, W // 2
        out.append(torch.zeros(1, c, H, W))
    return out


def record_all(mp):
    """{sequence name: [records]} of every walk and mode the golden file holds."""
    from dvc_amd import nets, ops
    with contextlib.redirect_stdout(io.StringIO()):
        cvn, warp, vgg = nets.ColorVidNet(7), nets.WarpNet(1), nets.VGG19_pytorch()
    seqs = {}
    x = torch.zeros(1, 7, 16, 24)       # the smallest map on which three stride-2 stages still leave 2 x 3
    for name, dual in (("cvn.inference.dual", True), ("cvn.inference.no_dual", False)):
        seqs[name] = _standins(mp, ops, dual=dual)
        cvn._forward(x)
    seqs["cvn.training"] = _standins(mp, ops)
    cvn._forward(x, saved={}, rstd={})
    seqs["cvn.training.backward"] = log = _standins(mp, ops)
    saved, rstd = {}, {}
    saved["ab"] = cvn._forward(x, saved=saved, rstd=rstd)
    saved.update(("rstd:" + k, v) for k, v in rstd.items())     # (as _CVNTrain.forward hands them over)
    log.append({"op": "-- _backward"})
    cvn._backward(saved, torch.zeros_like(saved["ab"]), {n for n, _ in cvn.named_parameters()}, True)
    for H, W in ((48, 80), (40, 64)):
        seqs[f"warp.heads.{H}x{W}"] = _standins(mp, ops)
        warp._heads(*_vgg_features(H, W))
    img = torch.zeros(1, 3, 32, 48)
    for keys in (ALL_VGG_TAPS, ["r34", "p3"]):
        for fused in (True, False):
            seqs[f"vgg.{'+'.join(keys)}.{'fused' if fused else 'unfused'}"] = _standins(mp, ops, pool_fusion=fused)
            vgg._forward(img, keys, True, False)
    seqs["vgg.training.backward"] = log = _standins(mp, ops)
    saved = {}
    outs = vgg._forward(img, ALL_VGG_TAPS, True, False, saved=saved)
    log.append({"op": "-- _input_grad"})
    vgg._input_grad(saved, {k: torch.zeros_like(o) for k, o in zip(ALL_VGG_TAPS, outs)}, True)
    return json.loads(json.dumps(seqs))     # (what a reader of the golden file gets: lists for tuples)


def dump(seqs, commit, path):
    """One record per line, so that a changed launch is one changed line."""
    with open(path, "w") as f:
        f.write('{\n "_commit": %s' % json.dumps(commit))
        for name, records in seqs.items():
            f.write(',\n "%s": [\n' % name + ",\n".join("  " + json.dumps(r, sort_keys=True) for r in records) + "\n ]")
        f.write("\n}\n")


if __name__ == "__main__":
    import subprocess

    import pytest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "deep-exemplar-based-video-colorization_amd"), root]
    head = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    with pytest.MonkeyPatch.context() as mp:
        dump(record_all(mp), head, sys.argv[1])
