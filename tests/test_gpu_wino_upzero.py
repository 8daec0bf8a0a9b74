"""The two-input Winograd launch (dvc_conv2d_winograd_dual) leaves out the transform positions that are exactly zero for an
input read through in_up == 2 (UPZ, csrc/conv_wino_kernel.h).  That must not change one bit of the output.

Reference: the SAME entry point fed the materialised upsample (`repeat_interleave` twice, in_up = 1): the launch then cannot
take the UPZ form and runs the full K loop, with the same plan (tile-block shape and split are forced through cfg / split_k,
and the output size is the same) and therefore the same summation order.  Every case asserts torch.equal.

Shapes: the entry point takes channel counts that are multiples of 8 (include/dvc_hip.h), so the smallest inputs are 8 + 8
channels (two 4-channel chunks each); a K range that holds exactly ONE up chunk — the first loop runs once — comes from the
splits instead: 16 + 8 channels at split 2 give the ranges [0, 3) (wholly up) and [3, 6) (one up chunk, then the short-cut).
The up input is 5 x 7, the short-cut 10 x 14: 5 x 7 output tiles, odd counts and partial tile blocks for every tile-block
shape.  The entry point has no residual input, so there is no such case.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 5, 7          # stored size of the up input; the short-cut and the output are 10 x 14


@pytest.fixture(scope="module")
def ops():
    from dvc_amd import ops as o
    return o


def _inputs(N, CA, CB, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    xA = torch.randn(N, CA, H, W, generator=g)
    xB = torch.randn(N, CB, 2 * H, 2 * W, generator=g)
    # exact zeros among the values (also a whole row, a whole column and a whole channel), negative values from randn
    xA[xA.abs() < 0.3] = 0.0
    xB[xB.abs() < 0.3] = 0.0
    xA[:, 1] = 0.0
    xA[:, :, 0, :] = 0.0
    xA[:, 2, :, W - 1] = 0.0
    w = torch.randn(Cout, CA + CB, 3, 3, generator=g) / ((CA + CB) * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    return xA.cuda(), xB.cuda(), w.cuda(), b.cuda()


def _dual(ops, xA, xB, u, b, *, in_upA, tr_idx, split, act, pad_mode):
    """dvc_conv2d_winograd_dual with the 64-channel x 32-tile workgroup shape's tile-block choice `tr_idx` (cfg 8 + index of
    1, 2, 4, 8 tile rows) and the split over input-channel chunks forced."""
    from dvc_amd import _lib
    lib = _lib.load()
    N, CA, HA, WA = xA.shape
    _, CB, HB, WB = xB.shape
    Cout = u.shape[0] * 32
    OH, OW = HB, WB
    common = dict(pad_mode=pad_mode, act=act, act_slope=0.2)
    dA = ops._conv_desc(N, CA, HA, WA, Cout, in_up=in_upA, cfg=8 + tr_idx, split_k=split, **common)
    dB = ops._conv_desc(N, CB, HB, WB, Cout, **common)
    ws = ops._workspace(xA.device, ops.CONV_WORKSPACE_BYTES, "conv")
    ops._bump_generation(ws)
    # the plan the launch will take (same planner, total channel count): the forced split must be the one that runs
    got_split, per_launch = ops._winograd_split(lib, ops._conv_desc(N, CA + CB, OH, OW, Cout, cfg=8 + tr_idx, split_k=split, **common),
                                                ws.numel())
    assert got_split == split and per_launch >= N
    out = torch.empty((N, Cout, OH, OW), device=xA.device, dtype=torch.float32)
    _lib.check(lib.dvc_conv2d_winograd_dual(ctypes.byref(dA), ctypes.byref(dB), ops._p(xA), ops._p(xB), ops._p(u), ops._p(b), None,
                                            ops._p(out), ctypes.c_void_p(ws.data_ptr()), ws.numel(), ops._stream()),
               "dvc_conv2d_winograd_dual")
    return out


# (N, CA, CB, Cout, tile-block index, split, act, pad_mode)
CASES = (
    # every tile-block shape (1, 2, 4, 8 tile rows of a 32-tile block), one and two channel blocks, unsplit
    [(1, 8, 8, co, ti, 1, 1, 0) for co in (64, 128) for ti in range(4)] +
    [
        (2, 8, 8, 64, 0, 1, 0, 0),       # batch 2, no activation
        (2, 8, 8, 64, 1, 2, 1, 0),       # split 2: [0, 2) is the up input, [2, 4) the short-cut — each range wholly in one part
        (2, 16, 8, 128, 1, 2, 0, 0),     # split 2, boundary inside the up part: [0, 3) up | [3, 6) ONE up chunk, then the short-cut
        (2, 16, 8, 64, 2, 3, 1, 0),      # split 3: [0, 2) [2, 4) up | [4, 6) short-cut
        (2, 16, 16, 64, 0, 3, 1, 0),     # split 3 straddling the boundary: [0, 3) up | [3, 6) one up + two short-cut | [6, 8)
        (1, 16, 16, 128, 3, 3, 0, 0),    # ... with the 8-row tile blocks and two channel blocks
        (2, 8, 16, 64, 1, 2, 1, 0),      # split 2: [0, 3) two up chunks and one short-cut | [3, 6)
        (1, 8, 8, 64, 1, 1, 1, 1),       # reflect padding: rows / columns 1 and 2 of a patch are still one stored element
        (2, 16, 8, 64, 2, 2, 0, 1),      # ... split, batch 2
    ]
)


@pytest.mark.parametrize("N,CA,CB,Cout,ti,split,act,pad_mode", CASES)
def test_upzero_bits(ops, N, CA, CB, Cout, ti, split, act, pad_mode):
    xA, xB, w, b = _inputs(N, CA, CB, Cout, seed=1000 * CA + 10 * CB + Cout + ti + split)
    u = ops.pack_winograd_weight(w)
    kw = dict(tr_idx=ti, split=split, act=act, pad_mode=pad_mode)
    got = _dual(ops, xA, xB, u, b, in_upA=2, **kw)
    up = xA.repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()
    want = _dual(ops, up, xB, u, b, in_upA=1, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all() and want.abs().max().item() > 0.1
    if act == 1:
        assert (want == 0).any() and (want > 0).any()
    else:
        assert (want < 0).any()
    assert torch.equal(got, want)


def test_upzero_matches_single_input_launch(ops):
    """... and the single-input Winograd launch on cat([up(x), s], 1) with the same workgroup shape, tile blocks and split: the
    same chunks in the same order, so the same bits."""
    N, CA, CB, Cout = 2, 16, 8, 128
    xA, xB, w, b = _inputs(N, CA, CB, Cout, seed=7)
    u = ops.pack_winograd_weight(w)
    got = _dual(ops, xA, xB, u, b, in_upA=2, tr_idx=1, split=2, act=1, pad_mode=0)
    x = torch.cat((xA.repeat_interleave(2, 2).repeat_interleave(2, 3), xB), 1).contiguous()
    want = ops.conv2d_winograd(x, u, b, act=1, act_slope=0.2, cfg=9, split_k=2)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
