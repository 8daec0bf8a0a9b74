"""CPU: the gradient guard without a device — the restatement tests/grad_guard_reference.py against
torch.nn.utils.clip_grad_norm_ and torch.optim.Adam on float64 tensors, with four seeded defects that must each lose their own
check by a wide margin; the plumbing of the four new entry points and their refusals before any launch; the tables the functional
API builds; every refusal of dvc_amd.optim.grad_norm / clip_grad_norm_ / GuardedAdam and of the two keywords on Adam and
CapturableAdam; and GuardedAdam's pickle / deepcopy / state_dict round trips."""
import copy
import ctypes
import math
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dvc_grad_norm", "dvc_adam_advance_guarded", "dvc_adam_step_guarded", "dvc_grad_scale")


def _grads(seed, sizes=(5, 1, 300, 4097), scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=gen) * scale).float() for n in sizes]


# ---- the restatement against torch
@pytest.mark.parametrize("scale, max_norm", [(1.0, 0.5), (1.0, 1e3), (1e-8, 1e-7), (1e3, 2.0)])
def test_restatement_matches_torch_clip_grad_norm(scale, max_norm):
    grads = _grads(1, scale=scale)
    ps = [torch.nn.Parameter(torch.zeros(g.numel(), dtype=torch.float64)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.double()
    want = torch.nn.utils.clip_grad_norm_(ps, max_norm).item()
    got = R.norm(grads)
    assert abs(got - want) <= 1e-14 * want
    c = R.coefficient(got, max_norm)
    assert (c == 1.0) == (want + 1e-6 <= max_norm)
    for p, g in zip(ps, grads):
        assert torch.allclose(p.grad, g.double() * c, rtol=1e-14, atol=0.0)


def test_restatement_sumsq_is_exact_on_integers():
    gen = torch.Generator().manual_seed(2)
    grads = [torch.randint(-2048, 2049, (n,), generator=gen).float() for n in (1, 3, 4095, 4097)]
    assert R.sumsq(grads) == float(sum(int((g.long() ** 2).sum()) for g in grads))
    assert R.norm([torch.tensor([3.0, 4.0])]) == 5.0 and R.norm([torch.ones(16384)]) == 128.0
    assert math.isnan(R.norm([torch.tensor([1.0, float("nan")])])) and R.norm([torch.tensor([1.0, -float("inf")])]) == math.inf


def _adam_sequence(grad_steps, defect=None, max_norm=0.5, **kw):
    """p after the guarded restatement has seen `grad_steps` (a list of per-tensor gradient lists), and its info per step."""
    sizes = [g.numel() for g in grad_steps[0]]
    states = [dict(p=torch.linspace(-1, 1, n), m=torch.zeros(n), v=torch.zeros(n), vmax=torch.zeros(n), t=0) for n in sizes]
    cfg = dict(lr=1e-2, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False)
    infos, skipped = [], 0
    for grads in grad_steps:
        states, _, info = R.guarded_step(states, grads, [cfg] * len(sizes), max_norm=max_norm, skipped=skipped, defect=defect, **kw)
        states = [dict(p=s["p"].float(), m=s["m"].float(), v=s["v"].float(), vmax=s["vmax"].float(), t=s["t"]) for s in states]
        skipped = info["skipped"]
        infos.append(info)
    return states, infos


def _torch_sequence(grad_steps, max_norm=0.5):
    """The same in torch, float64: clip_grad_norm_ then Adam.step, with the non-finite steps left out."""
    sizes = [g.numel() for g in grad_steps[0]]
    ps = [torch.nn.Parameter(torch.linspace(-1, 1, n).double()) for n in sizes]
    opt = torch.optim.Adam(ps, lr=1e-2, betas=(0.5, 0.999), eps=1e-8)
    for grads in grad_steps:
        if not all(bool(torch.isfinite(g).all()) for g in grads):
            continue
        for p, g in zip(ps, grads):
            p.grad = g.double()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    return ps, opt


def _steps_with_a_nan():
    steps = [_grads(10 + i, sizes=(5, 300)) for i in range(3)]
    steps[1][1][17] = float("nan")
    return steps


def test_restatement_steps_match_torch_and_skip_whole_steps():
    steps = _steps_with_a_nan()
    states, infos = _adam_sequence(steps)
    ps, opt = _torch_sequence(steps)
    assert [i["found_inf"] for i in infos] == [0, 1, 0] and [i["skipped"] for i in infos] == [0, 1, 1]
    assert [s["t"] for s in states] == [2, 2] == [int(opt.state[p]["step"]) for p in ps]
    for s, p in zip(states, ps):
        assert torch.allclose(s["p"].double(), p.detach(), rtol=0, atol=2e-6)      # (fp32 state between the restated steps)
    # skip_nonfinite=False: the flag stays down and the NaN goes through
    states, infos = _adam_sequence(steps, skip_nonfinite=False)
    assert [i["found_inf"] for i in infos] == [0, 0, 0] and [s["t"] for s in states] == [3, 3]
    assert bool(torch.isnan(states[1]["p"]).any())


# ---- seeded defects: each loses its own check by a wide margin
def test_defect_eps_dropped():
    grads = [torch.full((4,), 5e-7)]               # norm 1e-6: the 1e-6 of the denominator halves the coefficient
    n = R.norm(grads)
    good, bad = R.coefficient(n, 1e-7), R.coefficient(n, 1e-7, defect="eps_dropped")
    ps = [torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))]
    ps[0].grad = grads[0].double()
    torch.nn.utils.clip_grad_norm_(ps, 1e-7)
    want = (ps[0].grad[0] / grads[0].double()[0]).item()
    assert abs(good - want) <= 1e-12 * want and abs(bad - want) > 0.9 * want


def test_defect_no_clamp():
    grads = _grads(3)
    n = R.norm(grads)
    assert R.coefficient(n, 10 * n) == 1.0 and R.coefficient(n, 10 * n, defect="no_clamp") > 9.9


def test_defect_advance_on_skip():
    steps = _steps_with_a_nan()
    ps, _ = _torch_sequence(steps)
    good, _ = _adam_sequence(steps)
    bad, _ = _adam_sequence(steps, defect="advance_on_skip")
    assert [s["t"] for s in bad] == [3, 3]
    err = lambda states: max((s["p"].double() - p.detach()).abs().max().item() for s, p in zip(states, ps))     # noqa: E731
    # the defect uses step 3's bias correction for the second real step: lr / (1 - 0.5^3) against lr / (1 - 0.5^2), 14 % of an
    # update of order lr = 1e-2 — two orders above the 2e-6 the fp32 state between the restated steps costs
    assert err(good) <= 2e-6 and err(bad) > 2e-4


def test_defect_per_tensor_norm():
    steps = [_grads(20, sizes=(5, 300))]
    ps, _ = _torch_sequence(steps, max_norm=2.0)        # the small tensor alone is under 2.0 (or near it); the set is far over it
    good, _ = _adam_sequence(steps, max_norm=2.0)
    bad, _ = _adam_sequence(steps, defect="per_tensor_norm", max_norm=2.0)
    first = lambda states: (states[0]["m"].double() * 2).abs().max().item()        # noqa: E731  m after step 1 = (1 - b1) c g
    g = steps[0][0].double().abs().max().item()
    c_global = R.coefficient(R.norm(steps[0]), 2.0)
    assert abs(first(good) / g - c_global) <= 1e-6 and first(bad) / g > 3 * c_global


# ---- plumbing
def test_entry_points_in_header_table_and_exports():
    from dvc_amd import _lib, ops, optim
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(rf"\b{name}\(", hdr) and name in _lib.SIGNATURES and re.search(rf"\b{name}\b", out), name
    assert _lib.load().dvc_abi_version() == _lib.ABI_VERSION == 20 and "#define DVC_ABI_VERSION 20" in hdr     # purely additive
    assert ctypes.sizeof(_lib.DvcGradGuard) == optim.GUARD_DTYPE.itemsize == 24
    body = re.search(r"typedef struct DvcGradGuard \{(.*?)\} DvcGradGuard;\s*/\* 24 bytes \*/", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1] for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in _lib.DvcGradGuard._fields_] == list(optim.GUARD_DTYPE.names) == ["total_norm", "clip_coef", "found_inf", "skipped", "sumsq"]
    assert [optim.GUARD_DTYPE.fields[n][1] for n in names] == [0, 4, 8, 12, 16]
    assert "#define DVC_GRAD_NORM_KEEP_NONFINITE 1u" in hdr and ops.GRAD_NORM_KEEP_NONFINITE == 1
    assert ctypes.sizeof(_lib.DvcAdamTensor) == 80 and ctypes.sizeof(_lib.DvcAdamChunk) == 16 and ctypes.sizeof(_lib.DvcAdamAdvance) == 40
    src = open(os.path.join(ROOT, "deep-exemplar-based-video-colorization_amd", "csrc", "optim.hip")).read()
    assert "static_assert(sizeof(DvcGradGuard) == 24" in src and "#pragma clang fp contract(off)" in src


def test_c_entry_points_refuse_before_any_launch():
    from dvc_amd import _lib, ops
    lib = _lib.load()
    one = ctypes.c_void_p(64)
    inf = math.inf

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    for bad in (0.0, -1.0, -inf, math.nan):
        refused(lib.dvc_grad_norm(one, 1, one, 1, one, bad, 0, one, None), "max_norm")
        refused(lib.dvc_grad_norm(None, 0, None, 0, None, bad, 0, None, None), "max_norm")
    refused(lib.dvc_grad_norm(one, 1, one, 1, one, 1.0, 2, one, None), "unknown flags")
    refused(lib.dvc_grad_norm(one, -1, one, 1, one, 1.0, 0, one, None), "negative count")
    refused(lib.dvc_grad_norm(one, 1, one, -1, one, 1.0, 0, one, None), "negative count")
    refused(lib.dvc_grad_norm(None, 1, one, 1, one, 1.0, 0, one, None), "null table")
    refused(lib.dvc_grad_norm(one, 1, None, 1, one, 1.0, 0, one, None), "null table")
    refused(lib.dvc_grad_norm(one, 1, one, 1, one, 1.0, 0, None, None), "null guard")
    refused(lib.dvc_grad_norm(one, 1, one, 0, one, 1.0, 0, one, None), "no chunks")
    refused(lib.dvc_grad_norm(one, 1, one, 1, None, inf, 0, one, None), "null partials")
    assert lib.dvc_grad_norm(None, 0, None, 0, None, inf, 0, None, None) == 0           # nothing to do: a successful no-op
    for fn in (lib.dvc_adam_step_guarded, lib.dvc_grad_scale):
        refused(fn(one, -1, one, 1, one, None), "negative count")
        refused(fn(None, 1, one, 1, one, None), "null table")
        refused(fn(one, 1, None, 1, one, None), "null table")
        refused(fn(one, 1, one, 1, None, None), "null guard")
        refused(fn(one, 1, one, 0, one, None), "no chunks")
        assert fn(None, 0, None, 0, None, None) == 0
    refused(lib.dvc_adam_advance_guarded(one, one, -1, one, None), "negative count")
    refused(lib.dvc_adam_advance_guarded(None, one, 1, one, None), "null table")
    refused(lib.dvc_adam_advance_guarded(one, None, 1, one, None), "null table")
    refused(lib.dvc_adam_advance_guarded(one, one, 1, None, None), "null guard")
    assert lib.dvc_adam_advance_guarded(None, None, 0, None, None) == 0
    t80, t16, t40, t24 = (torch.zeros(n, dtype=torch.uint8) for n in (80, 16, 40, 24))
    for call in (lambda: ops.grad_norm(t80, 1, t16, 1, torch.zeros(1, dtype=torch.float64), 1.0, t24),
                 lambda: ops.adam_advance_guarded(t40, t80, 1, t24), lambda: ops.adam_step_guarded(t80, 1, t16, 1, t24),
                 lambda: ops.grad_scale(t80, 1, t16, 1, t24)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the functional API
def test_norm_tables_of_the_functional_api():
    from dvc_amd import optim
    C = optim.CHUNK
    grads = [torch.zeros(n) for n in (5, C + 1, 0, 2 * C)]
    tensors, chunks = optim.build_norm_tables(grads)
    assert (tensors.dtype, chunks.dtype) == (optim.TENSOR_DTYPE, optim.CHUNK_DTYPE) and len(tensors) == 4
    assert tensors["g"].tolist() == [g.data_ptr() for g in grads] and tensors["n"].tolist() == [5, C + 1, 0, 2 * C]
    for name in optim.TENSOR_DTYPE.names:
        if name not in ("g", "n"):
            assert not tensors[name].any(), name
    assert chunks["tensor"].tolist() == [0, 1, 1, 3, 3] and chunks["start"].tolist() == [0, 0, C, 0, C]


def test_functional_refusals():
    from dvc_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    assert optim.grad_norm([p]).item() == 0.0 and optim.clip_grad_norm_([p], 1.0).item() == 0.0      # no gradients: torch's 0.
    p.grad = torch.ones(3)
    for nt in (1, 1.0, math.inf, 0.5):
        with pytest.raises(NotImplementedError, match="norm_type"):
            optim.clip_grad_norm_([p], 1.0, norm_type=nt)
    for bad in (0.0, -1.0, math.nan, None):
        with pytest.raises(ValueError, match="max_norm"):
            optim.clip_grad_norm_([p], bad)
    with pytest.raises(NotImplementedError, match="tensor `max_norm`"):
        optim.clip_grad_norm_([p], torch.tensor(1.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.clip_grad_norm_(p, 1.0, norm_type=2, foreach=True)        # a single tensor, as torch accepts
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.grad_norm([p])
    assert torch.equal(p.grad, torch.ones(3))


# ---- the optimiser
def test_keywords_refused_by_adam_and_capturable_adam():
    from dvc_amd.optim import Adam, CapturableAdam
    w = [torch.nn.Parameter(torch.zeros(3))]
    for cls in (Adam, CapturableAdam):
        for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(skip_nonfinite=False), dict(max_grad_norm=1.0, skip_nonfinite=True)):
            with pytest.raises(NotImplementedError, match="GuardedAdam"):
                cls(w, **kw)
        cls(w)


def test_guarded_constructor():
    from dvc_amd.optim import CapturableAdam, GuardedAdam
    w = [torch.nn.Parameter(torch.zeros(3))]
    opt = GuardedAdam(w, lr=2e-4)
    assert isinstance(opt, CapturableAdam) and opt.max_grad_norm is None and opt.skip_nonfinite is True
    opt = GuardedAdam(w, lr=2e-4, max_grad_norm=0.5, skip_nonfinite=False)
    assert opt.max_grad_norm == 0.5 and opt.skip_nonfinite is False
    assert set(opt.param_groups[0]) == set(torch.optim.Adam(w, capturable=True).param_groups[0])      # attributes, not group keys
    with pytest.raises(TypeError):
        GuardedAdam(w, 1e-3, (0.9, 0.999), 1e-8, 0, False, None, False, True, False, None, False, 1.0)       # keyword only
    for bad in (0.0, -2.0, math.nan):
        with pytest.raises(ValueError, match="max_norm"):
            GuardedAdam(w, max_grad_norm=bad)
    with pytest.raises(NotImplementedError, match="tensor `max_norm`"):
        GuardedAdam(w, max_grad_norm=torch.tensor(1.0))
    with pytest.raises(ValueError, match="GuardedAdam: `capturable=False`"):
        GuardedAdam(w, capturable=False)
    for kw in ("maximize", "differentiable", "decoupled_weight_decay", "foreach", "fused"):
        with pytest.raises(NotImplementedError, match=kw):
            GuardedAdam(w, **{kw: True})
    assert opt.step() is None and len(opt.state) == 0          # nothing to do without gradients
    w[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="GuardedAdam.*no CPU fallback"):
        opt.step()
    assert len(opt.state) == 0
    with pytest.raises(RuntimeError, match="no guard record"):
        opt.last_grad_norm
    with pytest.raises(RuntimeError, match="no guard record"):
        opt.skipped_steps
    opt.mark_updated()


def _hand_state(p, t, seed):
    gen = torch.Generator().manual_seed(seed)
    return {"step": torch.tensor(float(t)), "exp_avg": torch.randn(p.shape, generator=gen), "exp_avg_sq": torch.rand(p.shape, generator=gen)}


def test_pickle_deepcopy_and_state_dict_round_trips():
    from dvc_amd.optim import CapturableAdam, GuardedAdam
    ps = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3, 4))]
    groups = lambda: [{"params": ps[:1]}, {"params": ps[1:], "lr": 4e-4}]          # noqa: E731
    opt = GuardedAdam(groups(), lr=2e-4, betas=(0.5, 0.999), max_grad_norm=0.25, skip_nonfinite=False)
    for i, p in enumerate(ps):
        opt.state[p] = _hand_state(p, 3, i)
    for twin in (pickle.loads(pickle.dumps(opt)), copy.deepcopy(opt)):
        assert type(twin) is GuardedAdam and twin.max_grad_norm == 0.25 and twin.skip_nonfinite is False
        assert [g["lr"] for g in twin.param_groups] == [2e-4, 4e-4]
        assert all(k.startswith("_dvc") is False or twin.__dict__[k] is None for k in twin.__dict__ if k.startswith("_dvc"))
        assert [st["step"].item() for st in twin.state.values()] == [3.0, 3.0]
    # the state dict is CapturableAdam's and torch's: no trace of the two options
    sd = opt.state_dict()
    ref = torch.optim.Adam(groups(), lr=2e-4, betas=(0.5, 0.999), capturable=True)
    assert sd["param_groups"] == ref.state_dict()["param_groups"]
    assert "max_grad_norm" not in sd and all("max_grad_norm" not in g and "skip_nonfinite" not in g for g in sd["param_groups"])
    again = torch.optim.Adam(groups(), lr=1.0, capturable=True)
    again.load_state_dict(sd)
    assert [g["lr"] for g in again.param_groups] == [2e-4, 4e-4]
    for p in ps:
        assert list(again.state[p]) == ["step", "exp_avg", "exp_avg_sq"] and again.state[p]["step"].item() == 3.0
        assert torch.equal(again.state[p]["exp_avg"], opt.state[p]["exp_avg"])
    # and back: torch's and CapturableAdam's dicts load, and the options are the constructor's
    mine = GuardedAdam(groups(), lr=1.0, max_grad_norm=7.0)
    mine.load_state_dict(again.state_dict())
    assert mine.max_grad_norm == 7.0 and mine.skip_nonfinite is True and [g["lr"] for g in mine.param_groups] == [2e-4, 4e-4]
    cap = CapturableAdam(groups(), lr=1.0)
    cap.load_state_dict(sd)
    mine.load_state_dict(cap.state_dict())
    assert all(mine.state[p]["step"].item() == 3.0 and mine.state[p]["step"].dtype == torch.float32 for p in ps)
    assert mine.state_dict()["state"].keys() == sd["state"].keys()
