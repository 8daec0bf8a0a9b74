"""CPU: dvc_amd.losses and dvc_loss_fwd / dvc_loss_bwd (csrc/loss.hip) without a device — the plumbing of the new entry points, the
table records against the numpy dtypes, every refusal of the C entry points before any launch (through never-dereferenced
pointers), the chunk table, the Python refusals that need no device, the drop-in boundary of utils.util next to a stand-in
reference tree, and the float64 restatement tests/losses_reference.py (what the GPU tests compare against) with its bound."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd")
REF_STANDIN = os.path.join(ROOT, "tests", "golden", "reference_tree")
NEW = ("dvc_loss_fwd", "dvc_loss_bwd")


# ---- plumbing
def _header_fields(hdr, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    return [n.split()[-1].strip("*") for n in names]


def test_entry_points_in_header_table_and_exports():
    from dvc_amd import _lib, losses, optim
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr) and name in _lib.SIGNATURES and re.search(r"\b%s\b" % name, out), name
        assert len(_lib.SIGNATURES[name][1]) == 8
    assert _lib.load().dvc_abi_version() == _lib.ABI_VERSION == 20 and "#define DVC_ABI_VERSION 20" in hdr
    assert int(re.search(r"#define DVC_LOSS_CHUNK (\d+)", hdr).group(1)) == losses.CHUNK == optim.CHUNK
    assert losses.CHUNK % 1024 == 0      # whole 16-byte passes of a 256-thread workgroup
    # the table records: csrc/loss.hip static_asserts their sizes, numpy writes them
    assert ctypes.sizeof(_lib.DvcLossTerm) == losses.TERM_DTYPE.itemsize == 80
    assert ctypes.sizeof(_lib.DvcLossChunk) == losses.CHUNK_DTYPE.itemsize == 16
    for struct, cls, dt in (("DvcLossTerm", _lib.DvcLossTerm, losses.TERM_DTYPE), ("DvcLossChunk", _lib.DvcLossChunk, losses.CHUNK_DTYPE)):
        assert _header_fields(hdr, struct) == [f[0] for f in cls._fields_] == list(dt.names), struct
        for name in dt.names:
            assert dt.fields[name][1] == getattr(cls, name).offset, (struct, name)
    assert [losses.TERM_DTYPE.fields[n][1] for n in losses.TERM_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76]
    assert [losses.CHUNK_DTYPE.fields[n][1] for n in losses.CHUNK_DTYPE.names] == [0, 4, 8]


def _term(**kw):
    """One valid DvcLossTerm row (addresses that nothing dereferences), with overrides."""
    from dvc_amd import losses
    row = dict(x=4096, t=0, w=0, dx=0, dt=0, n=5, plane=1, cpl=0, p=2, reserved=0, t_scalar=0.0, scale=1.0)
    row.update(kw)
    return np.array([tuple(row[k] for k in losses.TERM_DTYPE.names)], dtype=losses.TERM_DTYPE)


@pytest.mark.parametrize("entry", NEW)
def test_c_entry_points_refuse_before_any_launch(entry):
    from dvc_amd import _lib, losses
    lib = _lib.load()
    fn = getattr(lib, entry)
    one = ctypes.c_void_p(64)
    good = _term()

    def call(terms=one, host=good, n_terms=1, chunks=one, n_chunks=1, a=one, b=one):
        host_p = host if host is None or isinstance(host, ctypes.c_void_p) else ctypes.c_void_p(host.ctypes.data)
        return fn(terms, host_p, n_terms, chunks, n_chunks, a, b, None)

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    refused(call(n_terms=-1), "negative count")
    refused(call(n_chunks=-1), "negative count")
    refused(call(terms=None), "null table")
    refused(call(host=None), "null table")
    refused(call(chunks=None), "null table")
    refused(call(n_chunks=0), "no chunks for 1 terms")
    refused(call(host=_term(p=0)), "p = 0 is neither 1 nor 2")
    refused(call(host=_term(p=3)), "p = 3 is neither 1 nor 2")
    refused(call(host=_term(n=0)), "n = 0 is not positive")
    refused(call(host=_term(n=-4)), "n = -4 is not positive")
    refused(call(host=_term(x=0)), "null x")
    refused(call(host=_term(plane=0)), "plane = 0 is not positive")
    refused(call(host=_term(plane=-3)), "plane = -3 is not positive")
    refused(call(host=_term(n=24, plane=4, cpl=6)), "cpl = 6 is not a multiple of plane = 4")
    refused(call(host=_term(n=20, plane=4, cpl=8)), "n = 20 is not a multiple of cpl = 8")
    refused(call(host=_term(n=losses.CHUNK + 1)), "1 chunks for terms that cut into 2")
    refused(call(n_chunks=2), "2 chunks for terms that cut into 1")
    two = np.concatenate([_term(), _term(p=7)])
    refused(call(host=two, n_terms=2, n_chunks=2), "term 1: p = 7")
    if entry == "dvc_loss_fwd":
        refused(call(a=None), "null partials / values")
        refused(call(b=None), "null partials / values")
    else:
        refused(call(a=None), "null grad_total")        # (grad_values may be null: zeros)
    assert fn(None, None, 0, None, 0, None, None, None) == 0          # nothing to do: a successful no-op, no launch
    assert fn(one, one, 0, one, 5, one, one, None) == 0


def test_ops_wrappers_refuse_host_tables():
    from dvc_amd import ops
    z = torch.zeros(80, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.loss_fwd(z, z, 1, torch.zeros(16, dtype=torch.uint8), 1, torch.zeros(1, dtype=torch.float64), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.loss_bwd(z, z, 1, torch.zeros(16, dtype=torch.uint8), 1, torch.zeros(1))


# ---- the tables
def test_chunk_table_covers_every_element_once():
    from dvc_amd import losses
    C = losses.CHUNK
    sizes = [1, C - 1, C, C + 1, 2 * C + 1, 5, 3 * C]
    table = losses.chunk_table(sizes)
    assert table.dtype == losses.CHUNK_DTYPE and len(table) == sum(-(-n // C) for n in sizes) == 1 + 1 + 1 + 2 + 3 + 1 + 3
    seen = [np.zeros(n, dtype=np.int32) for n in sizes]
    for ti, start in zip(table["term"].tolist(), table["start"].tolist()):
        assert 0 <= ti < len(sizes) and start % C == 0 and 0 <= start < sizes[ti]       # inside its term: no chunk crosses one
        seen[ti][start:min(start + C, sizes[ti])] += 1          # (the kernel's extent: min(CHUNK, n - start))
    for n, s in zip(sizes, seen):
        assert (s == 1).all(), n
    assert (table["reserved"] == 0).all() and (np.diff(table["term"]) >= 0).all()
    # term k's chunks follow those of the terms before it, in order of start: what stage 2 of the forward relies on
    first = 0
    for k, n in enumerate(sizes):
        cnt = -(-n // C)
        assert table["term"][first:first + cnt].tolist() == [k] * cnt
        assert table["start"][first:first + cnt].tolist() == [j * C for j in range(cnt)]
        first += cnt


def test_build_tables_lays_out_the_records():
    from dvc_amd import losses
    terms, chunks = losses.build_tables([(4096, 8192, 0, 0, 0, 5, 1, 0, 2, 0.0, 0.25),
                                         (4100, 0, 12288, 16, 32, 2 * losses.CHUNK, 10, 30, 1, 0.5, -3.0)])
    assert terms.dtype == losses.TERM_DTYPE and terms.shape == (2,) and chunks["term"].tolist() == [0, 1, 1]
    assert terms["x"].tolist() == [4096, 4100] and terms["t"].tolist() == [8192, 0] and terms["w"].tolist() == [0, 12288]
    assert terms["dx"].tolist() == [0, 16] and terms["dt"].tolist() == [0, 32] and terms["n"].tolist() == [5, 2 * losses.CHUNK]
    assert terms["plane"].tolist() == [1, 10] and terms["cpl"].tolist() == [0, 30] and terms["p"].tolist() == [2, 1]
    assert terms["t_scalar"].tolist() == [0.0, 0.5] and terms["scale"].tolist() == [0.25, -3.0] and (terms["reserved"] == 0).all()


# ---- the Python refusals that need no device
def test_python_refusals_without_a_device():
    from dvc_amd import losses
    x = torch.zeros(2, 3, 4, 5)
    for fn in (losses.mse_loss, losses.l1_loss):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, torch.zeros_like(x))
        with pytest.raises(TypeError, match="float32"):
            fn(x.double())
        with pytest.raises(TypeError, match="target must be float32"):
            fn(x, x.half())
        with pytest.raises(NotImplementedError, match="broadcasting a target of shape"):
            fn(x, torch.zeros(1, 3, 4, 5))
        with pytest.raises(NotImplementedError, match="broadcasting a target of shape"):
            fn(x, torch.zeros(()))
        with pytest.raises(ValueError, match="no elements.*NaN"):
            fn(torch.zeros(2, 0, 4))
    for fn in (losses.weighted_mse_loss, losses.weighted_l1_loss):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x, torch.ones(2, 1, 4, 5))
        with pytest.raises(TypeError, match="weights must be float32"):
            fn(x, x, torch.ones(2, 1, 4, 5, dtype=torch.float64))
        with pytest.raises(NotImplementedError, match="weights that require grad"):
            fn(x, x, torch.ones(2, 1, 4, 5, requires_grad=True))
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):     # (not under no_grad: the mask is data)
            fn(x, x, torch.ones(2, 1, 4, 5, requires_grad=True))
        for bad in ((1, 1, 4, 5), (2, 3, 1, 5), (2, 1, 4, 1), (4, 5), (2, 3, 4, 1)):
            with pytest.raises(NotImplementedError, match="broadcasting weights of shape"):
                fn(x, x, torch.ones(bad))
        with pytest.raises(NotImplementedError, match="broadcasting weights of shape"):
            fn(torch.zeros(3, 4), torch.zeros(3, 4), torch.ones(1, 4))      # [B,1,H,W] is for 4-D inputs only
    with pytest.raises(ValueError, match="kind must be"):
        losses.fused([("huber", x, 0, None, 1.0)])
    with pytest.raises(ValueError, match="no terms"):
        losses.fused([])
    with pytest.raises(ValueError, match="term 1 is not"):
        losses.fused([("mse", x, 0, None, 1.0), ("mse", x, 0)])
    with pytest.raises(TypeError, match="scale must be a Python number"):
        losses.fused([("mse", x, 0, None, torch.tensor(1.0))])
    with pytest.raises(RuntimeError, match="term 0: input must be a ROCm device tensor"):
        losses.fused([("mse", x, 0, None, 1.0), ("l1", x, 0.5, None, 2.0)])
    with pytest.raises(TypeError, match="term 0: input must be float32"):
        losses.fused([("l1", x.double(), 0.5, None, 2.0), ("mse", x, 0, None, 1.0)])


# ---- the drop-in boundary
def test_utils_util_serves_the_four_losses_and_forwards_the_rest():
    code = textwrap.dedent(f'''
        import os, sys
        sys.dont_write_bytecode = True
        sys.path[:0] = [{PKG!r}, {REF_STANDIN!r}]
        import utils.util, dvc_amd.losses
        from utils.util import mse_loss, l1_loss, weighted_mse_loss, weighted_l1_loss, save_frames
        for name in ("mse_loss", "l1_loss", "weighted_mse_loss", "weighted_l1_loss"):
            assert getattr(utils.util, name) is getattr(dvc_amd.losses, name), name
        assert mse_loss is dvc_amd.losses.mse_loss and weighted_l1_loss is dvc_amd.losses.weighted_l1_loss
        assert save_frames.__module__ == "utils._reference_util"
        assert save_frames.__code__.co_filename == os.path.join({REF_STANDIN!r}, "utils", "util.py")
        import inspect
        assert str(inspect.signature(mse_loss)) == "(input, target=0)" == str(inspect.signature(l1_loss))
        assert str(inspect.signature(weighted_mse_loss)) == "(input, target, weights)" == str(inspect.signature(weighted_l1_loss))
        print("OK")
    ''')
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + "\n" + r.stderr


# ---- the restatement
CASES = [("mse", (7,), None, False), ("l1", (4097,), None, False), ("mse", (3, 2, 1, 5), (3, 1, 1, 5), False),
         ("l1", (2, 3, 2, 4), (2, 1, 2, 4), False), ("mse", (2, 2, 8, 520), (2, 2, 8, 520), False),
         ("l1", (2, 2, 8, 520), (2, 1, 8, 520), True), ("mse", (2, 3, 2, 4), (2, 1, 2, 4), True)]


def test_restatement_equals_torch_functional_in_float64():
    for seed, (kind, shape, _, _) in enumerate(CASES):
        x, t, _ = R.make_case(shape, seed)
        f = F.mse_loss if kind == "mse" else F.l1_loss
        x64 = x.double().requires_grad_(True)
        want = f(x64, t.double())
        (3 * want).backward()
        ref = R.term(kind, x, t, upstream=3.0)
        assert abs(ref["value64"] - want.item()) <= 1e-14 * abs(want.item()) and ref["A"] == ref["value64"]
        assert torch.allclose(ref["dx64"], x64.grad, rtol=1e-14, atol=0)
        zero = R.term(kind, x, 0)
        assert abs(zero["value64"] - f(x.double(), torch.zeros_like(x64)).item()) <= 1e-14 * zero["value64"]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_fp32_arithmetic_stays_inside_the_value_bound(case):
    """The bound leaves no case leaning on slack: the expression evaluated in fp32 (float64 sum) is inside it, for a tensor target,
    a scalar target and a scale; and a seeded defect (one fp16-grade rounding of d) is far outside."""
    kind, shape, mask, signed = CASES[case]
    x, t, w = R.make_case(shape, 10 + case, mask, signed)
    for target, scale in ((t, 1.0), (0, 1.0), (0.5, -0.3)):
        ref = R.term(kind, x, target, w, scale)
        got = R.fp32_composition(kind, x, target, w, scale)
        err = R.value_error(got, ref)
        print(kind, shape, mask, signed, scale, "error / (EPS A) =", err)
        assert R.value_within_bound(got, ref) and err <= R.C_VALUE
        assert ref["A"] >= abs(ref["value64"]) > 0
    bad = R.fp32_composition(kind, x.half().float(), t.half().float(), w)
    assert not R.value_within_bound(bad, R.term(kind, x, t, w))


def test_bound_constants_are_the_derived_ones():
    assert (R.C_VALUE, R.C_GRAD, R.EPS) == (6.0, 6.0, 2.0 ** -24)
