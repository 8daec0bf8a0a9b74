"""CPU: dvc_amd.optim.CapturableAdam and dvc_adam_advance (csrc/optim.hip) without a device — the plumbing of the new entry point
and its refusals before any launch; that dvc_amd.optim.Adam still refuses `capturable=True` and a tensor `lr`; the constructor;
the state_dict contract with torch.optim.Adam(capturable=True) in both directions on CPU-constructed dicts (torch's capturable
step itself needs a device, so the states are written by hand); the tables a rebuild writes; and the fingerprint that decides
whether a step rebuilds them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- plumbing
def test_entry_point_in_header_table_and_exports():
    from dvc_amd import _lib, optim
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bdvc_adam_advance\(", hdr) and "dvc_adam_advance" in _lib.SIGNATURES and re.search(r"\bdvc_adam_advance\b", out)
    assert _lib.load().dvc_abi_version() == _lib.ABI_VERSION == 20 and "#define DVC_ABI_VERSION 20" in hdr     # purely additive
    assert ctypes.sizeof(_lib.DvcAdamAdvance) == optim.ADVANCE_DTYPE.itemsize == 40
    body = re.search(r"typedef struct DvcAdamAdvance \{(.*?)\} DvcAdamAdvance;\s*/\* 40 bytes \*/", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.split()[-1].strip("*") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    assert names == [f[0] for f in _lib.DvcAdamAdvance._fields_] == list(optim.ADVANCE_DTYPE.names), names
    assert [optim.ADVANCE_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24, 32]
    restype, argtypes = _lib.SIGNATURES["dvc_adam_advance"]
    assert restype is ctypes.c_int and len(argtypes) == 4          # (advance, tensors, n_tensors, stream)
    # the step kernel's records did not move
    assert ctypes.sizeof(_lib.DvcAdamTensor) == 80 and ctypes.sizeof(_lib.DvcAdamChunk) == 16


def test_c_entry_point_refuses_before_any_launch():
    from dvc_amd import _lib, ops
    lib = _lib.load()
    one = ctypes.c_void_p(64)

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    refused(lib.dvc_adam_advance(one, one, -1, None), "negative count")
    refused(lib.dvc_adam_advance(None, one, 1, None), "null table")
    refused(lib.dvc_adam_advance(one, None, 1, None), "null table")
    assert lib.dvc_adam_advance(None, None, 0, None) == 0           # nothing to do: a successful no-op, no launch
    assert lib.dvc_adam_advance(one, one, 0, None) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_advance(torch.zeros(40, dtype=torch.uint8), torch.zeros(80, dtype=torch.uint8), 1)


# ---- the two classes' constructors
def test_plain_adam_still_refuses_capturable_and_tensor_lr():
    from dvc_amd.optim import Adam
    w = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError, match="capturable.*CapturableAdam"):
        Adam(w, capturable=True)
    with pytest.raises(NotImplementedError, match="tensor `lr`.*CapturableAdam"):
        Adam(w, lr=torch.tensor(1e-3))
    opt = Adam(w)
    assert opt.param_groups[0]["capturable"] is False
    opt.param_groups[0]["capturable"] = True
    w[0].grad = torch.zeros(3)
    with pytest.raises(NotImplementedError, match="capturable"):
        opt.step()


def test_constructor():
    from dvc_amd.optim import CapturableAdam
    w = [torch.nn.Parameter(torch.zeros(3))]
    for kw in ("maximize", "differentiable", "decoupled_weight_decay", "foreach", "fused"):
        with pytest.raises(NotImplementedError, match=kw):
            CapturableAdam(w, **{kw: True})
    with pytest.raises(ValueError, match="capturable=False"):
        CapturableAdam(w, capturable=False)
    with pytest.raises(NotImplementedError, match="betas"):
        CapturableAdam(w, betas=(torch.tensor(0.9), torch.tensor(0.999)))
    for kw, text in ((dict(lr=-1e-3), "Invalid learning rate"), (dict(eps=-1e-8), "Invalid epsilon value"),
                     (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0"), (dict(weight_decay=-1.0), "Invalid weight_decay value"),
                     (dict(lr=torch.zeros(2)), "one-element float32"), (dict(lr=torch.zeros((), dtype=torch.float64)), "one-element float32")):
        with pytest.raises(ValueError, match=text):
            CapturableAdam(w, **kw)
    lr = torch.tensor(2e-4)
    opt = CapturableAdam([{"params": w}, {"params": [torch.nn.Parameter(torch.zeros(2))], "lr": 4e-4}], lr=lr, betas=(0.5, 0.999))
    assert opt.param_groups[0]["lr"] is lr and opt.param_groups[1]["lr"] == 4e-4
    assert all(g["capturable"] is True for g in opt.param_groups)
    ref = torch.optim.Adam(w, capturable=True)
    assert set(opt.param_groups[0]) == set(ref.param_groups[0])
    with pytest.raises(RuntimeError, match="tensor `lr` must be a ROCm device tensor"):      # accepted at construction, refused at the step
        opt.step()
    # nothing to do without gradients; CPU tensors are refused and nothing is created or advanced
    opt = CapturableAdam(w, lr=2e-4)
    assert opt.step() is None and len(opt.state) == 0
    w[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert len(opt.state) == 0
    opt.mark_updated()              # no tables yet: nothing to bump, nothing raised


# ---- the state contract
def _hand_state(p, t, amsgrad, seed):
    gen = torch.Generator().manual_seed(seed)
    st = {"step": torch.tensor(float(t)), "exp_avg": torch.randn(p.shape, generator=gen), "exp_avg_sq": torch.rand(p.shape, generator=gen)}
    if amsgrad:
        st["max_exp_avg_sq"] = st["exp_avg_sq"] + 1
    return st


@pytest.mark.parametrize("amsgrad", [False, True])
def test_state_dict_round_trip_with_torch_capturable(amsgrad):
    from dvc_amd.optim import Adam, CapturableAdam
    ps = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3, 4))]
    groups = lambda: [{"params": ps[:1]}, {"params": ps[1:], "lr": 4e-4}]          # noqa: E731
    topt = torch.optim.Adam(groups(), lr=2e-4, betas=(0.5, 0.999), amsgrad=amsgrad, capturable=True)
    for i, p in enumerate(ps):
        topt.state[p] = _hand_state(p, 3, amsgrad, i)
    sd = topt.state_dict()
    mine = CapturableAdam(groups(), lr=1.0)
    mine.load_state_dict(sd)
    back = mine.state_dict()
    assert back.keys() == sd.keys() == {"state", "param_groups"} and back["param_groups"] == sd["param_groups"]
    assert [g["lr"] for g in mine.param_groups] == [2e-4, 4e-4] and all(g["capturable"] is True for g in mine.param_groups)
    keys = ["step", "exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])
    assert list(back["state"]) == [0, 1]
    for i, p in enumerate(ps):
        assert list(back["state"][i]) == keys == list(sd["state"][i])
        step = back["state"][i]["step"]
        assert step.dtype == torch.float32 and step.shape == () and step.device == p.device and step.item() == 3.0
        for k in keys[1:]:
            assert torch.equal(back["state"][i][k], sd["state"][i][k]) and back["state"][i][k].shape == p.shape
    # the reverse: torch.optim.Adam(capturable=True) loads what CapturableAdam saved
    again = torch.optim.Adam(groups(), lr=1.0, capturable=True)
    again.load_state_dict(back)
    assert [g["lr"] for g in again.param_groups] == [2e-4, 4e-4] and all(g["capturable"] for g in again.param_groups)
    for p in ps:
        assert list(again.state[p]) == keys and again.state[p]["step"].item() == 3.0 and again.state[p]["step"].shape == ()
    # a fresh CapturableAdam's own state_dict has torch's structure too
    fresh = CapturableAdam(groups(), lr=2e-4, betas=(0.5, 0.999), amsgrad=amsgrad)
    assert fresh.state_dict() == torch.optim.Adam(groups(), lr=2e-4, betas=(0.5, 0.999), amsgrad=amsgrad, capturable=True).state_dict()
    # a plain Adam's dict (CPU float32 step, capturable False) and a very old one (a Python number) load as well
    plain = Adam(groups(), lr=2e-4, betas=(0.5, 0.999), amsgrad=amsgrad)
    for i, p in enumerate(ps):
        plain.state[p] = _hand_state(p, 7, amsgrad, i)
    psd = plain.state_dict()
    psd["state"][1]["step"] = 7
    mine.load_state_dict(psd)
    assert all(g["capturable"] is True for g in mine.param_groups)
    for p in ps:
        step = mine.state[p]["step"]
        assert torch.is_tensor(step) and step.dtype == torch.float32 and step.device == p.device and step.item() == 7.0


# ---- the tables and the fingerprint
def _work(opt):
    """What CapturableAdam._collect hands to fingerprint / build_capturable_tables, written by hand for CPU tensors."""
    return [(g, p, p.grad, opt.state[p]) for g in opt.param_groups for p in g["params"] if p.grad is not None]


def _optimiser(amsgrad=False, lr=2e-4):
    from dvc_amd import optim
    C = optim.CHUNK
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (5, C + 1, 2 * C)]
    opt = optim.CapturableAdam([{"params": ps[:2]}, {"params": ps[2:], "lr": 4e-4, "weight_decay": 1e-2}], lr=lr, betas=(0.5, 0.999),
                               amsgrad=amsgrad)
    for i, p in enumerate(ps):
        p.grad = torch.zeros_like(p)
        opt.state[p] = _hand_state(p, 3, amsgrad, i)
    return opt, ps


@pytest.mark.parametrize("amsgrad", [False, True])
def test_tables_of_a_rebuild(amsgrad):
    from dvc_amd import optim
    lr = torch.tensor(2e-4)
    opt, ps = _optimiser(amsgrad, lr=lr)
    tensors, chunks, advance = optim.build_capturable_tables(_work(opt))
    assert (tensors.dtype, chunks.dtype, advance.dtype) == (optim.TENSOR_DTYPE, optim.CHUNK_DTYPE, optim.ADVANCE_DTYPE)
    assert len(tensors) == len(advance) == 3 and chunks["tensor"].tolist() == [0, 1, 1, 2, 2]
    for i, p in enumerate(ps):
        st = opt.state[p]
        assert tensors["p"][i] == p.data_ptr() and tensors["g"][i] == p.grad.data_ptr() and tensors["n"][i] == p.numel()
        assert tensors["m"][i] == st["exp_avg"].data_ptr() and tensors["v"][i] == st["exp_avg_sq"].data_ptr()
        assert tensors["vmax"][i] == (st["max_exp_avg_sq"].data_ptr() if amsgrad else 0)
        assert advance["step"][i] == st["step"].data_ptr() and (advance["beta1"][i], advance["beta2"][i]) == (0.5, 0.999)
        wd = 1e-2 if i == 2 else 0.0
        want = optim.adam_scalars(1, 1.0, 0.5, 0.999, 1e-8, wd)
        for name, w in list(zip(optim.TENSOR_DTYPE.names[6:], want))[2:]:
            assert tensors[name][i] == np.float32(w), name          # the five columns that do not depend on the step, rounded once
    assert (tensors["step_size"] == 0).all() and (tensors["inv_sqrt_bc2"] == 0).all()          # the device's to write
    assert advance["lr_tensor"].tolist() == [lr.data_ptr(), lr.data_ptr(), 0] and advance["lr"].tolist() == [0.0, 0.0, 4e-4]


def test_fingerprint_changes_exactly_when_the_tables_would():
    from dvc_amd import optim
    opt, ps = _optimiser(amsgrad=True)
    base = optim.fingerprint(_work(opt))
    same = lambda: optim.fingerprint(_work(opt)) == base            # noqa: E731
    assert same()
    # what a training iteration does between two steps leaves it alone: new values in the same storage, a bumped version
    with torch.no_grad():
        for p in ps:
            p.grad.add_(1.0)
            p.add_(1.0)
            opt.state[p]["step"] += 1
            opt.state[p]["exp_avg"].mul_(0.5)
    assert same()
    for g in opt.param_groups:
        g["lr"], g["betas"] = float(g["lr"]), tuple(g["betas"])     # equal values written again (a scheduler that did not move)
    assert same()
    opt.zero_grad(set_to_none=False)
    assert same()
    # every address, one at a time
    for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"):
        old = opt.state[ps[1]][key]
        opt.state[ps[1]][key] = old.clone()
        assert not same(), key
        opt.state[ps[1]][key] = old
        assert same()
    old = ps[1].grad
    ps[1].grad = old.clone()                        # a reallocated gradient
    assert not same()
    ps[1].grad = old
    assert same()
    old = ps[0].data
    ps[0].data = old.clone()                        # a parameter that moved
    assert not same()
    ps[0].data = old
    assert same()
    # every hyper-parameter, one at a time
    for key, value in (("lr", 1e-4), ("betas", (0.9, 0.999)), ("betas", (0.5, 0.99)), ("eps", 1e-6), ("weight_decay", 0.5), ("amsgrad", False)):
        old = opt.param_groups[1][key]
        opt.param_groups[1][key] = value
        assert not same(), key
        opt.param_groups[1][key] = old
        assert same()
    lr = torch.tensor(4e-4)                         # a tensor lr is fingerprinted by address: its value may change in place
    opt.param_groups[1]["lr"] = lr
    with_tensor = optim.fingerprint(_work(opt))
    assert with_tensor != base
    lr.mul_(0.5)
    assert optim.fingerprint(_work(opt)) == with_tensor
    opt.param_groups[1]["lr"] = lr.clone()
    assert optim.fingerprint(_work(opt)) != with_tensor
    opt.param_groups[1]["lr"] = 4e-4
    assert same()
    # a gradient that went to None
    old = ps[2].grad
    ps[2].grad = None
    assert not same()
    ps[2].grad = old
    assert same()
