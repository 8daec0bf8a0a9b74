"""CPU: dvc_amd.optim.Adam and dvc_adam_step (csrc/optim.hip) without a device — the plumbing of the new entry point and its
refusals before any launch; the chunk table; the float64 restatement tests/adam_reference.py (what the GPU tests compare against)
and its bound, checked on torch.optim.Adam's own CPU float32 step, which each seeded defect of the restatement loses; the
constructor's refusals; the state_dict contract with torch.optim.Adam in both directions."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- plumbing
def test_entry_point_in_header_table_and_exports():
    from dvc_amd import _lib, optim
    hdr = open(os.path.join(ROOT, "include", "dvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bdvc_adam_step\(", hdr) and "dvc_adam_step" in _lib.SIGNATURES and re.search(r"\bdvc_adam_step\b", out)
    assert _lib.load().dvc_abi_version() == _lib.ABI_VERSION == 20 and "#define DVC_ABI_VERSION 20" in hdr
    assert int(re.search(r"#define DVC_ADAM_CHUNK (\d+)", hdr).group(1)) == optim.CHUNK
    # the table records: the header states their sizes, csrc/optim.hip static_asserts them, numpy writes them
    assert ctypes.sizeof(_lib.DvcAdamTensor) == optim.TENSOR_DTYPE.itemsize == 80 and "/* 80 bytes */" in hdr
    assert ctypes.sizeof(_lib.DvcAdamChunk) == optim.CHUNK_DTYPE.itemsize == 16 and "/* 16 bytes */" in hdr
    body = re.search(r"typedef struct DvcAdamTensor \{(.*?)\} DvcAdamTensor;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in _lib.DvcAdamTensor._fields_] == list(optim.TENSOR_DTYPE.names), names
    assert optim.CHUNK % 1024 == 0      # whole 16-byte passes of a 256-thread workgroup


def test_c_entry_point_refuses_before_any_launch():
    from dvc_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)

    def refused(rc, text):
        assert rc != 0 and text in lib.dvc_last_error().decode(), lib.dvc_last_error()

    refused(lib.dvc_adam_step(one, -1, one, 1, None), "negative count")
    refused(lib.dvc_adam_step(one, 1, one, -1, None), "negative count")
    refused(lib.dvc_adam_step(None, 1, one, 1, None), "null table")
    refused(lib.dvc_adam_step(one, 1, None, 1, None), "null table")
    refused(lib.dvc_adam_step(one, 3, one, 0, None), "no chunks for 3 tensors")
    assert lib.dvc_adam_step(None, 0, None, 0, None) == 0          # nothing to do: a successful no-op, no launch
    assert lib.dvc_adam_step(one, 0, one, 5, None) == 0
    from dvc_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adam_step(torch.zeros(80, dtype=torch.uint8), 1, torch.zeros(16, dtype=torch.uint8), 1)


# ---- the chunk table
def test_chunk_table_covers_every_element_once():
    from dvc_amd import optim
    C = optim.CHUNK
    sizes = [0, 1, C - 1, C, C + 1, 2 * C + 3, 0, 5]
    table = optim.chunk_table(sizes)
    assert table.dtype == optim.CHUNK_DTYPE and len(table) == sum(-(-n // C) for n in sizes) == 0 + 1 + 1 + 1 + 2 + 3 + 0 + 1
    seen = [np.zeros(n, dtype=np.int32) for n in sizes]
    for ti, start in zip(table["tensor"].tolist(), table["start"].tolist()):
        assert 0 <= ti < len(sizes) and start % C == 0 and 0 <= start < sizes[ti]       # inside its tensor, never at or past n
        seen[ti][start:min(start + C, sizes[ti])] += 1          # (the kernel's extent: min(CHUNK, n - start))
    for n, s in zip(sizes, seen):
        assert (s == 1).all(), n
    assert (table["reserved"] == 0).all() and sorted(set(table["tensor"].tolist())) == [1, 2, 3, 4, 5, 7]      # none for n == 0
    assert (np.diff(table["tensor"]) >= 0).all()
    assert len(optim.chunk_table([])) == 0 and len(optim.chunk_table([0, 0])) == 0
    with pytest.raises(ValueError, match="negative element count"):
        optim.chunk_table([4, -1])


def test_build_tables_rounds_each_scalar_once():
    from dvc_amd import optim
    sc = optim.adam_scalars(3, 2e-4, 0.5, 0.999, 1e-8, 1e-2)
    tensors, chunks = optim.build_tables([(4096, 8192, 12288, 16384, 0, 5, sc), (4100, 8192, 12288, 16384, 20480, optim.CHUNK + 1, sc)])
    assert tensors.dtype == optim.TENSOR_DTYPE and tensors.shape == (2,) and chunks["tensor"].tolist() == [0, 1, 1]
    assert tensors["p"].tolist() == [4096, 4100] and tensors["vmax"].tolist() == [0, 20480] and tensors["n"].tolist() == [5, optim.CHUNK + 1]
    want = (2e-4 / (1 - 0.5 ** 3), 1 / np.sqrt(1 - 0.999 ** 3), 0.999, 0.5, 1 - 0.999, 1e-8, 1e-2, 0.0)
    for name, w in zip(optim.TENSOR_DTYPE.names[6:], want):
        assert tensors[name][0] == np.float32(w), name          # the double value, rounded once
    assert np.float32(1 - 0.999) != np.float32(1) - np.float32(0.999)      # (why 1 - beta2 is a table entry of its own)
    assert optim.vector_path(4096, 8192, 12288, 16384) and not optim.vector_path(4100, 8192, 12288, 16384)
    assert not optim.vector_path(4096, 8192, 12288, 16384, 20488)


# ---- the restatement and its bound against torch.optim.Adam's CPU float32 step
CONFIGS = {
    "train_py": dict(lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False),
    "weight_decay": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False),
    "amsgrad": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=True),
}
N, STEPS = 60000, 5


def _torch_cpu_run(cfg, seed, skip=()):
    """STEPS steps of torch.optim.Adam over two CPU tensors; the second gets no gradient on the steps in `skip`.  Yields per step and
    per tensor (t, the inputs of the step, torch's outputs)."""
    ps = [torch.nn.Parameter(R.make_p(N, seed + i)) for i in range(2)]
    opt = torch.optim.Adam(ps, foreach=False, **cfg)
    t = [0, 0]
    for it in range(1, STEPS + 1):
        records = []
        for i, p in enumerate(ps):
            if i == 1 and it in skip:
                p.grad = None
                continue
            p.grad = R.make_g(N, 100 * it + i + seed, like_sign_of=p if cfg["weight_decay"] else None)
            st = opt.state[p]
            zeros = torch.zeros(N)
            before = dict(p=p.detach().clone(), g=p.grad.clone(), m=st["exp_avg"].clone() if st else zeros,
                          v=st["exp_avg_sq"].clone() if st else zeros,
                          vmax=st["max_exp_avg_sq"].clone() if st and cfg["amsgrad"] else zeros)
            t[i] += 1
            records.append((i, t[i], before))
        opt.step()
        for i, ti, before in records:
            st = opt.state[ps[i]]
            assert st["step"].item() == ti
            yield it, i, ti, before, dict(p=ps[i].detach().clone(), m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone(),
                                         vmax=st.get("max_exp_avg_sq"))


def _worst(cfg, seed=0, skip=(), defect=None, shared_step=False):
    worst, masks = {}, True
    for it, i, ti, before, got in _torch_cpu_run(cfg, seed, skip):
        ref = R.step(before["p"], before["g"], before["m"], before["v"], before["vmax"], t=it if shared_step else ti, defect=defect, **cfg)
        c, ok = R.achieved(ref, before, got)
        masks = masks and ok
        for k, val in c.items():
            worst[k] = max(worst.get(k, 0.0), val)
    return worst, masks


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_restatement_and_bound_hold_for_torch_cpu_adam(name):
    worst, masks = _worst(CONFIGS[name], skip=(2, 3))
    print(name, worst)
    assert masks and R.within_bound(worst), (name, worst)


@pytest.mark.parametrize("defect", ["shared_step"] + list(R.DEFECTS))
def test_seeded_defects_of_the_restatement_are_caught(defect):
    """Defects seeded in the RESTATEMENT only: each makes it disagree with torch.optim.Adam beyond the bound."""
    cfg = CONFIGS["weight_decay" if defect == "wd_after_moments" else "train_py"]
    if defect == "shared_step":
        worst, _ = _worst(cfg, skip=(2, 3), shared_step=True)       # the parameter that sat out two steps is stepped with the others' t
        assert R.within_bound(_worst(cfg, skip=(), shared_step=True)[0])        # (nobody sits out: the shared count is right)
    else:
        worst, _ = _worst(cfg, defect=defect)
    assert not R.within_bound(worst) and worst["c_p"] > 100 * R.C_P, (defect, worst)


def test_bound_constants_are_the_derived_ones():
    assert (R.C_M, R.C_V, R.C_P) == (5.0, 7.0, 7.0) and max(R.C_M, R.C_V, R.C_P) <= 8 and R.EPS == 2.0 ** -24


# ---- the constructor
def test_constructor_refusals_and_value_checks():
    from dvc_amd.optim import Adam
    w = [torch.nn.Parameter(torch.zeros(3))]
    for kw in ("maximize", "capturable", "differentiable", "decoupled_weight_decay", "foreach", "fused"):
        with pytest.raises(NotImplementedError, match=kw):
            Adam(w, **{kw: True})
    with pytest.raises(NotImplementedError, match="tensor `lr`"):
        Adam(w, lr=torch.tensor(1e-3))
    with pytest.raises(NotImplementedError, match="betas"):
        Adam(w, betas=(torch.tensor(0.9), torch.tensor(0.999)))
    for kw, text in ((dict(lr=-1e-3), "Invalid learning rate"), (dict(eps=-1e-8), "Invalid epsilon value"),
                     (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0"), (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1"),
                     (dict(weight_decay=-1.0), "Invalid weight_decay value")):
        with pytest.raises(ValueError, match=text):
            Adam(w, **kw)
        with pytest.raises(ValueError, match=text):
            torch.optim.Adam(w, **kw)          # the same check, the same words
    opt = Adam(w, foreach=None, fused=False, maximize=False)           # accepted and ignored
    ref = torch.optim.Adam(w)
    assert set(opt.param_groups[0]) == set(ref.param_groups[0]) and opt.defaults["betas"] == (0.9, 0.999)
    # groups, as train.py builds the generator's optimiser
    a, b = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2))
    opt = Adam([{"params": [a]}, {"params": [b], "lr": 4e-4}], lr=2e-4, betas=(0.5, 0.999))
    assert [g["lr"] for g in opt.param_groups] == [2e-4, 4e-4] and all(g["betas"] == (0.5, 0.999) for g in opt.param_groups)
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))], "maximize": True})
    opt.param_groups[2]["params"][0].grad = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="maximize"):
        opt.step()                                                      # a flag that arrives with a group is refused at the step


def test_step_refuses_cpu_and_sparse_tensors():
    from dvc_amd.optim import Adam
    p = torch.nn.Parameter(torch.ones(4))
    opt = Adam([p])
    assert opt.step() is None and len(opt.state) == 0          # no gradient: nothing to do, no state, nothing refused
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(4)) and len(opt.state) == 0
    e = torch.nn.Parameter(torch.ones(4, 2))
    e.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 2), (4, 2))
    with pytest.raises(RuntimeError, match="does not support sparse gradients"):
        Adam([e]).step()
    calls = []
    p.grad = None
    assert Adam([p]).step(lambda: calls.append(torch.is_grad_enabled()) or 3.5) == 3.5 and calls == [True]


# ---- the state contract
def _three_cpu_steps(amsgrad):
    ps = [torch.nn.Parameter(R.make_p(n, 7 + n)) for n in (5, 12)]
    opt = torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:], "lr": 4e-4}], lr=2e-4, betas=(0.5, 0.999), amsgrad=amsgrad)
    for it in range(3):
        for p in ps:
            p.grad = R.make_g(p.numel(), it)
        opt.step()
    return ps, opt


@pytest.mark.parametrize("amsgrad", [False, True])
def test_state_dict_loads_from_torch_and_back(amsgrad):
    from dvc_amd.optim import Adam
    ps, topt = _three_cpu_steps(amsgrad)
    sd = topt.state_dict()
    mine = Adam([{"params": ps[:1]}, {"params": ps[1:]}], lr=1.0)
    mine.load_state_dict(sd)
    back = mine.state_dict()
    assert back.keys() == sd.keys() == {"state", "param_groups"} and back["param_groups"] == sd["param_groups"]
    assert [g["lr"] for g in mine.param_groups] == [2e-4, 4e-4] and mine.param_groups[0]["amsgrad"] is amsgrad
    keys = ["step", "exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])
    assert list(back["state"]) == [0, 1]
    for i in (0, 1):
        assert list(back["state"][i]) == keys == list(sd["state"][i])
        step = back["state"][i]["step"]
        assert step.dtype == torch.float32 and step.device.type == "cpu" and step.shape == () and step.item() == 3.0
        for k in keys[1:]:
            assert torch.equal(back["state"][i][k], sd["state"][i][k]) and back["state"][i][k].dtype == torch.float32
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # loaded, but it still will not step on the CPU
        mine.step()
    assert all(mine.state[p]["step"].item() == 3.0 for p in ps)           # a refused step advances nothing
    # the reverse: torch.optim.Adam loads what dvc_amd.optim.Adam saved, and steps
    again = torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:]}], lr=1.0)
    again.load_state_dict(back)
    assert [g["lr"] for g in again.param_groups] == [2e-4, 4e-4]
    again.step()
    assert all(again.state[p]["step"].item() == 4.0 for p in ps)
    # a fresh dvc_amd.optim.Adam's own state_dict has torch's structure too
    fresh, ref = Adam(ps, lr=2e-4, betas=(0.5, 0.999)), torch.optim.Adam(ps, lr=2e-4, betas=(0.5, 0.999))
    assert fresh.state_dict() == ref.state_dict()
    ref.load_state_dict(fresh.state_dict())


def test_schedulers_drive_the_group_lr():
    from dvc_amd.optim import Adam
    p = torch.nn.Parameter(torch.zeros(2))
    opt = Adam([p], lr=2e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    lrs = []
    for _ in range(4):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()                      # (no gradient: a no-op; the scheduler only needs to see the call)
        sched.step()
    assert lrs == [2e-4, 2e-4, 1e-4, 1e-4]
