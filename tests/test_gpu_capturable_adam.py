"""GPU: dvc_amd.optim.CapturableAdam / dvc_adam_advance (csrc/optim.hip).  The device-written scalars against optim.adam_scalars
within 1 fp32 ulp, with everything else in the table bit-identical to what was uploaded; three consecutive steps per configuration
held to the float64 restatement tests/adam_reference.py at its own bound, fed the path's own previous state; the same bits from
dvc_adam_step on a host-built table carrying the device's scalars; two launches and no upload while nothing moves, exactly one
rebuild when something does; a captured step replayed three times, with and without the table upload inside the capture, bit for
bit against eager steps; mark_updated; and dvc_amd.optim.Adam unchanged beside it.

Sizes 1, 3, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 5 plus one parameter that is a view 1 element into a buffer (the dword
path), betas (0.5, 0.999), (0.9, 0.999) and (0.0, 0.999)."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

BETAS = [(0.5, 0.999), (0.9, 0.999), (0.0, 0.999)]
SENTINEL = 12345.678
VIEW_N = 4097


def _sizes():
    from dvc_amd import optim
    C = optim.CHUNK
    assert C == 4096
    return [1, 3, C - 1, C, C + 1, 2 * C + 5]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _params(seed=0):
    """The six sizes, then the view: -> (parameters, the view's sentinel-filled buffer)."""
    params = [torch.nn.Parameter(R.make_p(n, seed + i, device="cuda")) for i, n in enumerate(_sizes())]
    buf = torch.full((VIEW_N + 8,), SENTINEL, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + VIEW_N]
    view.copy_(R.make_p(VIEW_N, seed + 50, device="cuda"))
    params.append(torch.nn.Parameter(view))
    assert params[-1].data_ptr() == buf.data_ptr() + 4
    return params, buf


def _clones(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


def _sentinels_intact(buf):
    want = torch.full((1,), SENTINEL).view(torch.int32).item()
    bits = buf.view(torch.int32)
    return bool((bits[:1] == want).all()) and bool((bits[1 + VIEW_N:] == want).all())


def _make_grads(opt, params, seed):
    out = []
    for i, p in enumerate(params):
        wd = _group_of(opt, p)["weight_decay"] != 0
        out.append(R.make_g(p.numel(), seed + i, like_sign_of=p if wd else None, device="cuda").view_as(p))
    return out


def _group_of(opt, p):
    for g in opt.param_groups:
        if any(q is p for q in g["params"]):
            return g
    raise KeyError


def _cfg(group):
    cfg = {k: group[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad")}
    if torch.is_tensor(cfg["lr"]):
        cfg["lr"] = float(cfg["lr"].item())             # (the TEST reads it; the optimiser never does)
    return cfg


def _snapshot(opt, p):
    st = opt.state.get(p, {})
    z = torch.zeros_like(p)
    return dict(p=p.detach().clone(), m=st["exp_avg"].clone() if st else z, v=st["exp_avg_sq"].clone() if st else z,
                vmax=st["max_exp_avg_sq"].clone() if "max_exp_avg_sq" in st else z, t=int(st["step"].item()) if st else 0)


def _step_and_check(opt, params, label, worst=None):
    """One opt.step() over `params` (their .grad is set; None: the parameter sits out), every stepped tensor held to the bound
    against the restatement fed the state from BEFORE the step; the others bitwise unchanged.  -> the t each tensor was stepped with."""
    worst = {} if worst is None else worst
    before = [_snapshot(opt, p) for p in params]
    grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
    cfgs = [_cfg(_group_of(opt, p)) for p in params]
    opt.step()
    ts = []
    for p, b, g, cfg in zip(params, before, grads, cfgs):
        st = opt.state.get(p, {})
        if g is None:
            assert _bits_equal(p.detach(), b["p"]), label
            if st:
                assert _bits_equal(st["exp_avg"], b["m"]) and _bits_equal(st["exp_avg_sq"], b["v"]) and st["step"].item() == b["t"], label
            ts.append(None)
            continue
        t = b["t"] + 1
        assert st["step"].is_cuda and st["step"].dtype == torch.float32 and st["step"].shape == () and st["step"].item() == t, label
        ref = R.step(b["p"], g, b["m"], b["v"], b["vmax"], t=t, **cfg)
        c, masks = R.achieved(ref, b, dict(p=p.detach(), m=st["exp_avg"], v=st["exp_avg_sq"], vmax=st.get("max_exp_avg_sq")))
        for k, val in c.items():
            worst[k] = max(worst.get(k, 0.0), val)
        assert masks and R.within_bound(c), (label, tuple(p.shape), t, c)
        ts.append(t)
    return ts


@contextlib.contextmanager
def _count():
    """Calls of the two launch wrappers and of the upload helper, in order."""
    from dvc_amd import ops, optim
    calls = []
    real = (ops.adam_advance, ops.adam_step, optim.CapturableAdam._upload)

    def advance(advance_table, tensor_table, n_tensors):
        calls.append(("advance", n_tensors))
        return real[0](advance_table, tensor_table, n_tensors)

    def step(tensor_table, n_tensors, chunk_table, n_chunks):
        calls.append(("step", n_tensors))
        return real[1](tensor_table, n_tensors, chunk_table, n_chunks)

    def upload(self, work, key, capturing):
        calls.append(("upload", len(work)))
        return real[2](self, work, key, capturing)

    ops.adam_advance, ops.adam_step, optim.CapturableAdam._upload = advance, step, upload
    try:
        yield calls
    finally:
        ops.adam_advance, ops.adam_step, optim.CapturableAdam._upload = real


# ---- the scalars dvc_adam_advance writes
def _col(records, name):
    """The bytes of one column of a structured array."""
    return np.ascontiguousarray(records[name]).tobytes()


def _ulps(a, b):
    """|a - b| in units in the last place, for positive finite float32 arrays."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert (a > 0).all() and (b > 0).all() and np.isfinite(a).all() and np.isfinite(b).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("tensor_lr", [False, True])
@pytest.mark.parametrize("betas", BETAS)
def test_advance_alone_writes_two_columns_and_the_step(betas, tensor_lr):
    """dvc_adam_advance alone on an uploaded table, for t = 1, 2, 3, 1000 and 100000 (the step preloaded with t - 1): `step` ends
    exactly t; step_size and inv_sqrt_bc2 are within 1 fp32 ulp of optim.adam_scalars(...) rounded to fp32; every other byte of the
    three tables is the uploaded one.  The 1 ulp is reasoned, not measured: the device's double pow may differ from libm's by a few
    double ulps, which can move the one rounding to fp32 by at most one place.

    Measured on the MI355X: of the 420 values checked (6 cases x 5 steps x 7 tensors x 2 columns), none was not bit-equal to the
    host's (the run prints the count per case)."""
    from dvc_amd import ops, optim
    params, _ = _params(seed=200)
    lr = torch.full((), 2e-4, device="cuda") if tensor_lr else 2e-4
    opt = optim.CapturableAdam([{"params": params[0::2]}, {"params": params[1::2], "lr": 4e-4, "weight_decay": 1e-2}], lr=lr, betas=betas,
                               amsgrad=True)
    work = []
    for g in opt.param_groups:
        for p in g["params"]:
            p.grad = torch.zeros_like(p)
            opt.state[p] = dict(step=torch.zeros((), device="cuda"), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p),
                                max_exp_avg_sq=torch.zeros_like(p))
            work.append((g, p, p.grad, opt.state[p]))
    tensors, chunks, advance = optim.build_capturable_tables(work)
    sent = np.concatenate([tensors.view(np.uint8), chunks.view(np.uint8), advance.view(np.uint8)])
    t_bytes, c_bytes = tensors.nbytes, chunks.nbytes
    off = 0
    for t in (1, 2, 3, 1000, 100000):
        table = torch.from_numpy(sent.copy()).cuda()
        for w in work:
            w[3]["step"].fill_(float(t - 1))
        ops.adam_advance(table[t_bytes + c_bytes:], table, len(work))
        got = table.cpu().numpy()
        assert all(w[3]["step"].item() == float(t) for w in work), t
        assert np.array_equal(got[t_bytes:], sent[t_bytes:]), t                        # the chunk and advance records
        back = got[:t_bytes].view(optim.TENSOR_DTYPE)
        for name in optim.TENSOR_DTYPE.names:
            if name not in ("step_size", "inv_sqrt_bc2"):
                assert _col(back, name) == _col(tensors, name), (t, name)
        want = np.array([optim.adam_scalars(t, float(np.float32(2e-4)) if tensor_lr and w[0] is opt.param_groups[0] else w[0]["lr"],
                                            betas[0], betas[1], w[0]["eps"], w[0]["weight_decay"])[:2] for w in work], dtype=np.float32)
        d0, d1 = _ulps(back["step_size"], want[:, 0]), _ulps(back["inv_sqrt_bc2"], want[:, 1])
        off += int((d0 != 0).sum() + (d1 != 0).sum())
        assert d0.max() <= 1 and d1.max() <= 1, (t, d0, d1)
    print(f"advance scalars, betas {betas}, tensor lr {tensor_lr}: {off} of {2 * 5 * len(work)} values not bit-equal to the host's")


# ---- steps against the float64 restatement
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("betas", BETAS)
def test_three_steps_meet_the_bound(betas, weight_decay, amsgrad):
    from dvc_amd.optim import CapturableAdam
    params, buf = _params(seed=210)
    opt = CapturableAdam([{"params": params[0::2]}, {"params": params[1::2], "lr": 4e-4}], lr=2e-4, betas=betas, weight_decay=weight_decay,
                         amsgrad=amsgrad)
    worst = {}
    for it in (1, 2, 3):
        for p, g in zip(params, _make_grads(opt, params, 100 * it)):
            p.grad = g
        assert _step_and_check(opt, params, (betas, weight_decay, amsgrad, it), worst) == [it] * len(params)
    assert _sentinels_intact(buf)
    print(betas, weight_decay, amsgrad, worst)


def test_tensor_lr_resumed_count_and_a_parameter_that_sits_out():
    from dvc_amd.optim import CapturableAdam
    params, buf = _params(seed=220)
    lr = torch.full((), 2e-4, device="cuda")
    opt = CapturableAdam(params, lr=lr, betas=(0.5, 0.999))
    for p, g in zip(params, _make_grads(opt, params, 1)):
        p.grad = g
    assert _step_and_check(opt, params, "first") == [1] * 7
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.tensor(1000.0)               # a CPU step, as a plain Adam saves it: moved to the device on load
    opt.load_state_dict(sd)
    assert all(opt.state[p]["step"].is_cuda for p in params) and opt.param_groups[0]["lr"].is_cuda
    lr = opt.param_groups[0]["lr"]                      # (load_state_dict deep-copies the groups: the tensor the optimiser reads now)
    seen = []
    for it in (1, 2, 3):
        if it == 2:
            lr.mul_(0.5)                                # in place: no rebuild, and the next step uses it
        for i, (p, g) in enumerate(zip(params, _make_grads(opt, params, 10 * it))):
            p.grad = None if (i == 4 and it == 2) else g
        with _count() as calls:
            seen.append(_step_and_check(opt, params, ("resumed", it)))
        assert [c[0] for c in calls] == ["upload", "advance", "step"]          # new gradients every time here
    assert seen == [[1001] * 7, [1002] * 4 + [None] + [1002] * 2, [1003] * 4 + [1002] + [1003] * 2]
    assert _sentinels_intact(buf)


# ---- the same kernel on the same scalars gives the same bits
def test_step_kernel_on_a_host_table_with_the_devices_scalars():
    from dvc_amd import ops, optim
    params, _ = _params(seed=230)
    twins = _clones(params)
    opt = optim.CapturableAdam(params, lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-2)
    m = [torch.zeros_like(p) for p in twins]
    v = [torch.zeros_like(p) for p in twins]
    for it in (1, 2):
        grads = _make_grads(opt, params, 300 * it)
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()
        res = opt._dvc_resident
        back = res.table.cpu().numpy()[:res.n_t * optim.TENSOR_DTYPE.itemsize].view(optim.TENSOR_DTYPE)
        entries = [(q.data_ptr(), g.data_ptr(), mi.data_ptr(), vi.data_ptr(), 0, q.numel(), tuple(float(back[name][i]) for name in optim.TENSOR_DTYPE.names[6:]))
                   for i, (q, g, mi, vi) in enumerate(zip(twins, grads, m, v))]
        tensors, chunks = optim.build_tables(entries)
        for name in optim.TENSOR_DTYPE.names[6:]:
            assert _col(tensors, name) == _col(back, name), name
        table = torch.from_numpy(np.concatenate([tensors.view(np.uint8), chunks.view(np.uint8)])).cuda()
        ops.adam_step(table, len(tensors), table[tensors.nbytes:], len(chunks))
        for p, q, mi, vi in zip(params, twins, m, v):
            st = opt.state[p]
            assert _bits_equal(p.detach(), q.detach()) and _bits_equal(st["exp_avg"], mi) and _bits_equal(st["exp_avg_sq"], vi), (it, p.shape)


# ---- resident tables
def test_unchanged_addresses_are_two_launches_and_one_rebuild_per_change():
    from dvc_amd.optim import CapturableAdam
    params, buf = _params(seed=240)
    opt = CapturableAdam(params, lr=2e-4, betas=(0.5, 0.999))
    static = [torch.zeros_like(p) for p in params]
    for p, s in zip(params, static):
        p.grad = s

    def next_step(it, expect):
        for s, g in zip(static, _make_grads(opt, params, 400 * it)):
            s.copy_(g)                                  # new values at the same addresses
        torch.cuda.synchronize()
        allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
        with _count() as calls:
            opt.step()
        grew = torch.cuda.memory_stats()["allocation.all.allocated"] - allocs
        assert [c[0] for c in calls] == expect, (it, calls)
        return grew

    next_step(1, ["upload", "advance", "step"])
    assert next_step(2, ["advance", "step"]) == 0       # exactly two launches: no copy, no allocation
    assert next_step(3, ["advance", "step"]) == 0
    static[2] = static[2].clone()                       # a reallocated .grad
    params[2].grad = static[2]
    next_step(4, ["upload", "advance", "step"])
    assert next_step(5, ["advance", "step"]) == 0
    opt.param_groups[0]["lr"] = 1e-4                    # what a scheduler does
    next_step(6, ["upload", "advance", "step"])
    assert next_step(7, ["advance", "step"]) == 0
    params[5].grad = None
    next_step(8, ["upload", "advance", "step"])
    assert next_step(9, ["advance", "step"]) == 0
    assert [int(opt.state[p]["step"].item()) for p in params] == [9] * 5 + [7, 9]
    # and the steps taken from resident tables are right ones: two more, checked against the restatement
    params[5].grad = static[5]
    for it in (10, 11):
        for s, g in zip(static, _make_grads(opt, params, 400 * it)):
            s.copy_(g)
        with _count() as calls:
            assert _step_and_check(opt, params, ("resident", it)) == [it] * 5 + [it - 2, it]
        assert [c[0] for c in calls] == (["upload"] if it == 10 else []) + ["advance", "step"]
    assert _sentinels_intact(buf)


def test_a_refused_step_advances_nothing():
    from dvc_amd.optim import CapturableAdam
    params, _ = _params(seed=250)
    opt = CapturableAdam(params, lr=2e-4)
    for p, g in zip(params, _make_grads(opt, params, 1)):
        p.grad = g
    opt.step()
    before = [_snapshot(opt, p) for p in params]
    opt.state[params[6]]["exp_avg"] = opt.state[params[6]]["exp_avg"].double()
    with _count() as calls:
        with pytest.raises(TypeError, match="CapturableAdam: state `exp_avg`"):
            opt.step()
    assert calls == []
    opt.state[params[6]]["exp_avg"] = opt.state[params[6]]["exp_avg"].float()
    for p, b in zip(params, before):
        assert opt.state[p]["step"].item() == 1 and _bits_equal(p.detach(), b["p"])
    assert _step_and_check(opt, params, "after the refusal") == [2] * 7


# ---- graphs
def _eager_twin(params, grads_per_step, **kw):
    """Eager steps on clones with the given gradient values -> (twins, optimiser)."""
    from dvc_amd.optim import CapturableAdam
    twins = _clones(params)
    lr = kw.pop("lr")
    opt = CapturableAdam(twins, lr=lr.clone() if torch.is_tensor(lr) else lr, **kw)
    for grads in grads_per_step:
        for q, g in zip(twins, grads):
            q.grad = g.clone()
        opt.step()
    return twins, opt


def _same_state(params, opt, twins, ref, step):
    for p, q in zip(params, twins):
        a, b = opt.state[p], ref.state[q]
        assert _bits_equal(p.detach(), q.detach()) and _bits_equal(a["exp_avg"], b["exp_avg"]) and _bits_equal(a["exp_avg_sq"], b["exp_avg_sq"])
        if "max_exp_avg_sq" in b:
            assert _bits_equal(a["max_exp_avg_sq"], b["max_exp_avg_sq"])
        assert a["step"].item() == b["step"].item() == step


@pytest.mark.parametrize("upload_captured", [False, True])
def test_captured_step_replays_bit_for_bit(upload_captured):
    """One warm-up step on a side stream, one step() captured (a straight line: [copy,] advance, step), three replays with the static
    gradients rewritten in place between them, against four eager steps on clones.  upload_captured: the captured step is the FIRST
    of an optimiser that loaded the warmed-up state, so the table upload is itself a node of the graph — and its lr is a device
    tensor, halved in place before the last replay."""
    from dvc_amd.optim import CapturableAdam
    params, buf = _params(seed=260)
    kw = dict(betas=(0.5, 0.999), weight_decay=1e-2, amsgrad=True)
    lr = torch.full((), 2e-4, device="cuda") if upload_captured else 2e-4
    opt = CapturableAdam(params, lr=lr, **kw)
    grads = [_make_grads(opt, params, 500 * it) for it in (1, 2, 3, 4)]
    if upload_captured:
        grads[3] = [g * 0.5 for g in grads[3]]
    twins, ref = _eager_twin(params, grads[:3], lr=lr, **kw)
    if upload_captured:
        ref.param_groups[0]["lr"].mul_(0.5)
    for q, g in zip(twins, grads[3]):
        q.grad = g.clone()
    ref.step()

    static = [g.clone() for g in grads[0]]
    for p, s in zip(params, static):
        p.grad = s
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                      # the warm-up: creates the state
    side.synchronize()
    if upload_captured:
        fresh = CapturableAdam(params, lr=lr, **kw)
        fresh.load_state_dict(opt.state_dict())
        opt = fresh
        lr = opt.param_groups[0]["lr"]                  # (load_state_dict deep-copies the groups: the tensor this optimiser reads)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _count() as calls:
        with torch.cuda.graph(graph):
            opt.step()
    assert [c[0] for c in calls] == (["upload"] if upload_captured else []) + ["advance", "step"]
    assert (opt._dvc_resident.pinned is not None) == upload_captured and opt._dvc_resident.captured
    torch.cuda.synchronize()
    assert all(opt.state[p]["step"].item() == 1 for p in params)           # a capture runs nothing
    versions = [p._version for p in params]
    for it in (1, 2, 3):
        for s, g in zip(static, grads[it]):
            s.copy_(g)
        if upload_captured and it == 3:
            lr.mul_(0.5)
        graph.replay()
        opt.mark_updated()
    torch.cuda.synchronize()
    _same_state(params, opt, twins, ref, 4)
    assert all(p._version >= v0 + 3 for p, v0 in zip(params, versions))
    assert _sentinels_intact(buf)
    # an eager step after the replays goes on from the device's count
    for s, g in zip(static, _make_grads(opt, params, 2500)):
        s.copy_(g)
    assert _step_and_check(opt, params, "eager after replays") == [5] * 7


def test_capture_refuses_to_create_state():
    from dvc_amd.optim import CapturableAdam
    params, _ = _params(seed=270)
    opt = CapturableAdam(params, lr=2e-4)
    for p, g in zip(params, _make_grads(opt, params, 1)):
        p.grad = g
    torch.cuda.synchronize()
    graph, other = torch.cuda.CUDAGraph(), torch.zeros(8, device="cuda")
    with _count() as calls:
        with torch.cuda.graph(graph):
            other.add_(1.0)
            with pytest.raises(RuntimeError, match="no state yet"):
                opt.step()
    torch.cuda.synchronize()
    assert calls == [] and len(opt.state) == 0
    assert _step_and_check(opt, params, "eager after the refusal") == [1] * 7


# ---- the plain Adam beside it
def test_plain_adam_unchanged_and_still_uncapturable():
    """dvc_amd.optim.Adam and CapturableAdam on clones: where the device's two scalars are bit-equal to the host's (checked per step
    and per tensor), the two classes run the same kernel on the same table values and must end bit-identical."""
    from dvc_amd import optim
    params, _ = _params(seed=280)
    twins = _clones(params)
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-2)
    plain, cap = optim.Adam(params, **kw), optim.CapturableAdam(twins, **kw)
    compared = 0
    for it in (1, 2, 3):
        grads = _make_grads(plain, params, 600 * it)
        for p, q, g in zip(params, twins, grads):
            p.grad, q.grad = g, g.clone()
        plain.step()
        cap.step()
        res = cap._dvc_resident
        back = res.table.cpu().numpy()[:res.n_t * optim.TENSOR_DTYPE.itemsize].view(optim.TENSOR_DTYPE)
        host = np.array(optim.adam_scalars(it, 2e-4, 0.5, 0.999, 1e-8, 1e-2)[:2], dtype=np.float32)
        for i, (p, q) in enumerate(zip(params, twins)):
            a, b = plain.state[p], cap.state[q]
            assert a["step"].device.type == "cpu" and a["step"].item() == b["step"].item() == it
            if back["step_size"][i] == host[0] and back["inv_sqrt_bc2"][i] == host[1]:
                compared += 1
                assert _bits_equal(p.detach(), q.detach()) and _bits_equal(a["exp_avg"], b["exp_avg"]) and _bits_equal(a["exp_avg_sq"], b["exp_avg_sq"])
            else:                                       # (a 1-ulp scalar: the twin goes its own way from here; resynchronise it)
                q.data.copy_(p.detach())
                b["exp_avg"].copy_(a["exp_avg"])
                b["exp_avg_sq"].copy_(a["exp_avg_sq"])
    print(f"plain Adam beside CapturableAdam: {compared} of 21 tensor-steps had bit-equal scalars and were compared")
    assert compared >= 1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="cannot be captured into a graph"):
            plain.step()
    torch.cuda.synchronize()
    assert all(plain.state[p]["step"].item() == 3 for p in params)
