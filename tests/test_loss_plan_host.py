"""CPU: dvc_amd.losses.Plan and dvc_loss_plan_check / _fwd / _bwd (csrc/loss_plan.hip) without a device — the plumbing of the new
entry points, the DvcPlanTerm record against the ctypes and numpy layouts, every refusal of dvc_loss_plan_check (through
never-dereferenced pointers), the launch entry points' own refusals, the tables and the fingerprint, the Python refusals that need
no device, `fused`'s unchanged refusal of the new kinds, and the float64 restatement tests/loss_plan_reference.py with its bounds."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_plan_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dvc_loss_plan_check": 4, "dvc_loss_plan_fwd": 8, "dvc_loss_plan_bwd": 9}


# ---- plumbing
def _header_fields(hdr, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    return [n.split()[-1].strip("*") for n in names]


def test_entry_points_record_and_abi_version():
    from dvc_amd import _lib, losses, ops
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    version_script = open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), "csrc", "exports.map")).read()
    assert "global: dvc_*;" in version_script           # the map exports by prefix: the new names need no line of their own
    for name, argc in NEW.items():
        assert re.search(r"\b%s\(" % name, hdr) and re.search(r"\b%s\b" % name, exported), name
        assert len(_lib.SIGNATURES[name][1]) == argc
    assert _lib.load().dvc_abi_version() == _lib.ABI_VERSION == 20 and "#define DVC_ABI_VERSION 20" in hdr      # purely additive
    # the record: csrc/loss_plan.hip static_asserts its size and that it begins with a DvcLossTerm; numpy writes it
    assert ctypes.sizeof(_lib.DvcPlanTerm) == losses.PLAN_TERM_DTYPE.itemsize == 112
    assert "static_assert(sizeof(DvcPlanTerm) == 112" in open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), "csrc",
                                                                           "loss_plan.hip")).read()
    names = [f[0] for f in _lib.DvcPlanTerm._fields_]
    assert _header_fields(hdr, "DvcPlanTerm") == names == list(losses.PLAN_TERM_DTYPE.names)
    for name in names:
        assert losses.PLAN_TERM_DTYPE.fields[name][1] == getattr(_lib.DvcPlanTerm, name).offset, name
    assert [losses.PLAN_TERM_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80, 88, 96, 104, 108]
    old = [f[0] for f in _lib.DvcLossTerm._fields_]
    assert [n if n != "reserved" else "kind" for n in old] == names[:len(old)]
    for o, n in zip(old, names):
        assert getattr(_lib.DvcLossTerm, o).offset == getattr(_lib.DvcPlanTerm, n).offset
    for kind, number in losses.PLAN_KINDS.items():
        assert int(re.search(r"#define DVC_LOSS_KIND_%s (\d+)" % {"l1": "L1", "mse": "MSE", "mean": "MEAN", "rel": "REL"}[kind],
                             hdr).group(1)) == number
    assert ops.loss_plan_scratch_doubles(3, 10, 2) == 2 * 10 + 2 + 2 * 3
    assert "(2 * (n_chunks) + (n_ychunks) + 2 * (n_terms))" in hdr


def _row(**kw):
    """One valid DvcPlanTerm row (addresses that nothing dereferences), with overrides."""
    from dvc_amd import losses
    row = dict(x=4096, t=0, w=0, dx=0, dt=0, n=5, plane=1, cpl=0, p=2, kind=2, t_scalar=0.0, scale=1.0, y=0, dy=0, n_y=0, c=0.0, slot=0)
    row.update(kw)
    return np.array([tuple(row[k] for k in losses.PLAN_TERM_DTYPE.names)], dtype=losses.PLAN_TERM_DTYPE)


def _rel(**kw):
    return _row(**dict(dict(kind=4, p=2, y=8192, n_y=3, c=1.0), **kw))


def test_plan_check_refuses_everything_on_the_host():
    from dvc_amd import _lib, losses
    lib = _lib.load()

    def check(host, n_chunks=1, n_ychunks=0, n_terms=None):
        ptr = None if host is None else ctypes.c_void_p(host.ctypes.data)
        return lib.dvc_loss_plan_check(ptr, len(host) if n_terms is None else n_terms, n_chunks, n_ychunks)

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    assert check(_row()) == 0 and check(_rel(), 1, 1) == 0 and check(_row(kind=3, p=1)) == 0 and check(_row(kind=1, p=1)) == 0
    assert check(None, 0, 0, n_terms=0) == 0 and check(_row(), 7, 3, n_terms=0) == 0        # nothing to check
    refused(check(_row(), n_terms=-1), "negative count")
    refused(check(_row(), n_chunks=-1), "negative count")
    refused(check(_row(), n_ychunks=-1), "negative count")
    refused(check(None, n_terms=1), "null table")
    refused(check(_row(), n_chunks=0), "no chunks for 1 terms")
    for kind in (0, 5, -1):
        refused(check(_row(kind=kind)), "kind = %d is outside 1..4" % kind)
    refused(check(_row(kind=1, p=2)), "p = 2 does not belong to kind 1")
    refused(check(_row(kind=2, p=1)), "p = 1 does not belong to kind 2")
    refused(check(_row(kind=3, p=2)), "p = 2 does not belong to kind 3")
    refused(check(_rel(p=1), 1, 1), "p = 1 does not belong to kind 4")
    refused(check(_row(p=0)), "p = 0 does not belong")
    refused(check(_row(n=0)), "n = 0 is not positive")
    refused(check(_row(n=-4)), "n = -4 is not positive")
    refused(check(_row(x=0)), "null x")
    refused(check(_row(plane=0)), "plane = 0 is not positive")
    refused(check(_row(n=24, plane=4, cpl=6)), "cpl = 6 is not a multiple of plane = 4")
    refused(check(_row(n=20, plane=4, cpl=8)), "n = 20 is not a multiple of cpl = 8")
    refused(check(_row(n=losses.CHUNK + 1)), "1 chunks for terms that cut into 2")
    refused(check(_row(), n_chunks=2), "2 chunks for terms that cut into 1")
    # the relativistic kind
    refused(check(_rel(y=0), 1, 1), "a relativistic term with a null y")
    refused(check(_rel(n_y=0), 1, 1), "n_y = 0 is not positive")
    refused(check(_rel(n_y=-2), 1, 1), "n_y = -2 is not positive")
    refused(check(_rel(t=64), 1, 1), "takes no target and no weights")
    refused(check(_rel(w=64), 1, 1), "takes no target and no weights")
    refused(check(_rel(slot=1), 1, 1), "slot = 1 is outside [0, 1)")
    refused(check(_rel(slot=-1), 1, 1), "slot = -1 is outside [0, 1)")
    refused(check(np.concatenate([_rel(), _row(), _rel()]), 3, 2), "term 2: slot = 0 is term 0's")
    assert check(np.concatenate([_rel(), _row(), _rel(slot=1)]), 3, 2) == 0
    refused(check(_rel(), 1, 0), "0 y chunks for relativistic terms that cut into 1")
    refused(check(_rel(n_y=losses.CHUNK + 1), 1, 1), "1 y chunks for relativistic terms that cut into 2")
    refused(check(_row(), 1, 1), "1 y chunks for relativistic terms that cut into 0")
    refused(check(_row(y=64)), "belong to a relativistic term")
    refused(check(_row(dy=64)), "belong to a relativistic term")
    refused(check(_row(kind=3, p=1, n_y=2)), "belong to a relativistic term")
    refused(check(np.concatenate([_row(), _row(kind=9)]), 2), "term 1: kind = 9")


@pytest.mark.parametrize("entry", ["dvc_loss_plan_fwd", "dvc_loss_plan_bwd"])
def test_launch_entry_points_refuse_counts_and_null_pointers_before_any_launch(entry):
    from dvc_amd import _lib
    lib = _lib.load()
    fn, one = getattr(lib, entry), ctypes.c_void_p(64)
    tail = (one, one) if entry.endswith("fwd") else (one, one, one)

    def call(terms=one, n_terms=1, chunks=one, n_chunks=1, n_ychunks=0, tail=tail):
        return fn(terms, n_terms, chunks, n_chunks, n_ychunks, *tail, None)

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    refused(call(n_terms=-1), "negative count")
    refused(call(n_chunks=-1), "negative count")
    refused(call(n_ychunks=-1), "negative count")
    refused(call(terms=None), "null table")
    refused(call(chunks=None), "null table")
    refused(call(n_chunks=0), "no chunks for 1 terms")
    if entry.endswith("fwd"):
        refused(call(tail=(None, one)), "null scratch / values")
        refused(call(tail=(one, None)), "null scratch / values")
    else:
        refused(call(tail=(None, one, one)), "null scratch / grad_total")
        refused(call(tail=(one, None, one)), "null scratch / grad_total")       # (grad_values may be null: zeros)
    assert call(terms=None, n_terms=0, chunks=None, n_chunks=0, tail=(None,) * len(tail)) == 0      # a successful no-op, no launch


def test_ops_wrappers_refuse_host_tables():
    from dvc_amd import ops
    z, c = torch.zeros(112, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.loss_plan_fwd(z, 1, c, 1, 0, torch.zeros(4, dtype=torch.float64), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.loss_plan_bwd(z, 1, c, 1, 0, torch.zeros(4, dtype=torch.float64), torch.zeros(1))
    with pytest.raises(RuntimeError, match="DvcPlanTerm records"):
        ops.loss_plan_check(np.zeros(1, dtype=np.float64), 1, 0)
    with pytest.raises(RuntimeError, match="kind = 0 is outside"):
        ops.loss_plan_check(_row(kind=0), 1, 0)


# ---- the tables and the fingerprint
ENTRIES = [(1, 4096, 8192, 0, 0, 0, 5, 1, 0, 0.0, 0.25, 0, 0, 0, 0.0),
           (4, 4100, 0, 0, 16, 0, 2 * 4096 + 3, 1, 0, 0.0, 0.5, 12288, 32, 4097, -1.0),
           (3, 6000, 0, 7000, 0, 0, 60, 10, 30, 0.5, -3.0, 0, 0, 0, 0.0),
           (4, 12288, 0, 0, 0, 0, 7, 1, 0, 0.0, 0.5, 4100, 0, 1, 1.0)]


def test_build_plan_tables_lays_out_records_and_both_chunk_ranges():
    from dvc_amd import _lib, losses
    terms, chunks, n_c, n_yc = losses.build_plan_tables(ENTRIES)
    assert terms.dtype == losses.PLAN_TERM_DTYPE and terms.shape == (4,) and chunks.dtype == losses.CHUNK_DTYPE
    assert (n_c, n_yc) == (1 + 3 + 1 + 1, 2 + 1) and len(chunks) == n_c + n_yc
    assert chunks["term"].tolist() == [0, 1, 1, 1, 2, 3] + [1, 1, 3]
    assert chunks["start"].tolist() == [0, 0, 4096, 8192, 0, 0] + [0, 4096, 0]
    assert terms["kind"].tolist() == [1, 4, 3, 4] and terms["p"].tolist() == [1, 2, 1, 2] and terms["slot"].tolist() == [0, 0, 0, 1]
    assert terms["x"].tolist() == [4096, 4100, 6000, 12288] and terms["y"].tolist() == [0, 12288, 0, 4100]
    assert terms["dx"].tolist() == [0, 16, 0, 0] and terms["dy"].tolist() == [0, 32, 0, 0] and terms["n_y"].tolist() == [0, 4097, 0, 1]
    assert terms["c"].tolist() == [0.0, -1.0, 0.0, 1.0] and terms["scale"].tolist() == [0.25, 0.5, -3.0, 0.5]
    assert terms["plane"].tolist() == [1, 1, 10, 1] and terms["cpl"].tolist() == [0, 0, 30, 0] and terms["t_scalar"].tolist()[2] == 0.5
    lib = _lib.load()
    assert lib.dvc_loss_plan_check(ctypes.c_void_p(terms.ctypes.data), 4, n_c, n_yc) == 0       # what Plan uploads passes the check


def test_fingerprint_changes_when_and_only_when_an_entry_field_does():
    from dvc_amd import losses
    base = losses.plan_fingerprint(ENTRIES)
    assert base == losses.plan_fingerprint([tuple(e) for e in ENTRIES]) == losses.plan_fingerprint([list(e) for e in ENTRIES])
    assert hash(base) == hash(losses.plan_fingerprint(list(ENTRIES)))
    changed = {"kind": (0, 2), "x": (1, 4104), "t": (2, 8196), "w": (3, 7004), "dx": (4, 64), "dt": (5, 64), "n": (6, 6),
               "plane": (7, 5), "cpl": (8, 60), "t_scalar": (9, 0.25), "scale": (10, 0.125), "y": (11, 12292), "dy": (12, 48),
               "n_y": (13, 4096), "c": (14, 0.5)}
    for k in range(len(ENTRIES)):
        for name, (col, value) in changed.items():
            other = [list(e) for e in ENTRIES]
            assert other[k][col] != value
            other[k][col] = value
            assert losses.plan_fingerprint(other) != base, (k, name)
    assert losses.plan_fingerprint(ENTRIES[:3]) != base and losses.plan_fingerprint(ENTRIES[::-1]) != base


# ---- the Python refusals that need no device
def test_plan_refusals_without_a_device():
    from dvc_amd import losses
    plan = losses.Plan()
    x = torch.zeros(2, 3, 4, 5)
    with pytest.raises(ValueError, match="no terms"):
        plan([])
    with pytest.raises(ValueError, match="term 1 is not"):
        plan([("mse", x, 0, None, 1.0), ("mse", x, 0)])
    with pytest.raises(ValueError, match="term 0: kind must be one of 'l1', 'mse', 'mean', 'rel'"):
        plan([("huber", x, 0, None, 1.0)])
    with pytest.raises(ValueError, match="kind must be one of"):
        plan([(4, x, 0, None, 1.0)])
    for kind in ("l1", "mse", "mean"):      # `fused`'s refusals, by the same types
        with pytest.raises(RuntimeError, match="term 0: input must be a ROCm device tensor"):
            plan([(kind, x, 0, None, 1.0)])
        with pytest.raises(TypeError, match="input must be float32"):
            plan([(kind, x.double(), 0, None, 1.0)])
        with pytest.raises(TypeError, match="scale must be a Python number"):
            plan([(kind, x, 0, None, torch.tensor(1.0))])
        with pytest.raises(TypeError, match="target must be a tensor of input's shape or a Python number"):
            plan([(kind, x, "0", None, 1.0)])
        with pytest.raises(NotImplementedError, match="broadcasting a target of shape"):
            plan([(kind, x, torch.zeros(1, 3, 4, 5), None, 1.0)])
        with pytest.raises(NotImplementedError, match="weights that require grad"):
            plan([(kind, x, x, torch.ones(2, 1, 4, 5, requires_grad=True), 1.0)])
        with pytest.raises(NotImplementedError, match="broadcasting weights of shape"):
            plan([(kind, x, x, torch.ones(2, 3, 1, 1), 1.0)])
        with pytest.raises(ValueError, match="no elements.*NaN"):
            plan([(kind, torch.zeros(2, 0, 4), 0, None, 1.0)])
    y = torch.zeros(7)
    with pytest.raises(TypeError, match="c must be a Python number"):
        plan([("rel", x, y, None, 1.0)])
    with pytest.raises(TypeError, match="c must be a Python number"):
        plan([("rel", x, y, torch.tensor(1.0), 1.0)])
    with pytest.raises(TypeError, match="c must be a Python number"):
        plan([("rel", x, y, True, 1.0)])
    with pytest.raises(TypeError, match="y must be a float32 device tensor"):
        plan([("rel", x, 0, 1.0, 1.0)])
    with pytest.raises(TypeError, match="y must be float32"):
        plan([("rel", x, y.double(), 1.0, 1.0)])
    with pytest.raises(TypeError, match="input must be float32"):
        plan([("rel", x.half(), y, 1.0, 1.0)])
    with pytest.raises(ValueError, match="y has no elements"):
        plan([("rel", x, torch.zeros(0), 1.0, 1.0)])
    with pytest.raises(ValueError, match="the input has no elements"):
        plan([("rel", torch.zeros(0), y, 1.0, 1.0)])
    with pytest.raises(TypeError, match="scale must be a Python number"):
        plan([("rel", x, y, 1.0, None)])
    with pytest.raises(RuntimeError, match="input must be a ROCm device tensor; the HIP reduction has no CPU fallback"):
        plan([("rel", x, y, 1.0, 0.5)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.relativistic_loss(x, y, -1.0)
    assert plan.uploads == 0
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="n_terms_hint must be a positive integer"):
            losses.Plan(n_terms_hint=bad)


def test_fused_still_refuses_the_new_kinds():
    from dvc_amd import losses
    x = torch.zeros(4)
    for term in (("mean", x, 0, None, 1.0), ("rel", x, x, 1.0, 1.0)):
        with pytest.raises(ValueError, match="kind must be 'mse' or 'l1'"):
            losses.fused([term])
    assert losses.KINDS == {"mse": 2, "l1": 1}


# ---- the restatement and its bounds
def _case(n, n_y, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), torch.randn(n_y, generator=g) + 0.3


@pytest.mark.parametrize("n,n_y,c", [(5, 1, 1.0), (4097, 7, -1.0), (1023, 4097, 1.0), (64, 64, 0.0)])
def test_rel_restatement_is_torchs_float64_and_fp32_arithmetic_stays_inside_the_bound(n, n_y, c):
    x, y = _case(n, n_y, 3 * n + n_y)
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    want = R.torch_rel(x64, y64, c, 0.5)
    (3 * want).backward()
    ref = R.rel_term(x, y, c, 0.5, upstream=3.0)
    assert abs(ref["value64"] - want.item()) <= 1e-13 * abs(want.item())
    assert torch.allclose(ref["dx64"], x64.grad, rtol=1e-12, atol=1e-300)
    assert torch.allclose(torch.full_like(y64, ref["dy64"]), y64.grad, rtol=1e-9, atol=1e-18)      # (sum d cancels: a looser rtol)
    got = R.rel_fp32_composition(x, y, c, 0.5)
    ev, _, _ = R.rel_errors(got, None, None, ref)
    print(n, n_y, c, "fp32 composition: error / bound =", ev)
    assert ev <= 1.0 and ref["value_bound"] < 1e-5 * abs(ref["value64"])        # inside, and the bound is an fp32-grade one
    lit = R.torch_rel(x, y, c, 0.5).item()
    assert abs(lit - ref["value64"]) <= R.torch_rel_bound(x, y, c, 0.5)
    # seeded defects are far outside: the mean over the wrong count, and an fp16-grade mean
    bad = R.rel_fp32_composition(x, y * (n_y / (n_y + 1.0)), c, 0.5)
    assert R.rel_errors(bad, None, None, ref)[0] > 1.0
    assert R.rel_errors(R.rel_fp32_composition(x, y.half().float(), c, 0.5), None, None, ref)[0] > 1.0


def test_mean_restatement_and_bound():
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(2, 3, 2, 5, generator=g), torch.randn(2, 3, 2, 5, generator=g)
    w = torch.randn(2, 1, 2, 5, generator=g)
    x64 = x.double().requires_grad_(True)
    want = R._f32(-0.3) * ((x64 - t.double()) * w.double().expand_as(x64)).mean()       # (the table carries the scale as fp32)
    (2 * want).backward()
    ref = R.mean_term(x, t, w, -0.3, upstream=2.0)
    assert abs(ref["value64"] - want.item()) <= 1e-13 * ref["A"] and ref["A"] > abs(ref["value64"])
    assert torch.allclose(ref["dx64"], x64.grad, rtol=1e-13, atol=0)
    fp32 = float(torch.tensor(float(((x - t) * w.expand_as(x)).double().sum()) * R._f32(-0.3) / x.numel(), dtype=torch.float32))
    assert abs(fp32 - ref["value64"]) <= R.mean_value_bound(ref)
    assert abs(float(-0.3 * ((x - t).abs() * w.expand_as(x)).mean()) - ref["value64"]) > R.mean_value_bound(ref)     # |.| is another term
    assert R.mean_grad_error(ref["dx64"].float(), ref) <= 1.0 < R.C_MEAN_GRAD


def test_bound_constants_are_the_derived_ones():
    assert (R.C_VALUE, R.C_GRAD, R.C_MEAN_VALUE, R.C_MEAN_GRAD, R.SLACK, R.EPS) == (6.0, 6.0, 4.0, 3.0, 1.0625, 2.0 ** -24)
