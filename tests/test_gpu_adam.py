"""GPU: dvc_amd.optim.Adam / dvc_adam_step (csrc/optim.hip) held, step by step, to the float64 restatement tests/adam_reference.py
at the bound derived there (C_M, C_V, C_P = 5, 7, 7 roundings) — fed the state the HIP path itself holds before each step — over
sizes around CHUNK, hyper-parameter configurations, a resumed step count, per-parameter steps, every misalignment of p, g, m, v,
vmax behind sentinels, many tensors in one launch, independence and reproducibility, non-finite gradients, zero_grad both ways,
a side stream, the version counter, the capture refusal, the state_dict interchange with torch.optim.Adam on the device, StepLR,
and two training iterations of ColorVidNet."""
import contextlib
import io
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

TRAIN_PY = dict(lr=2e-4, betas=(0.5, 0.999))


def _chunk():
    from dvc_amd import optim
    return optim.CHUNK


def _sizes():
    C = _chunk()
    return [1, 2, 3, 4, 5, 7, C - 1, C, C + 1, 2 * C + 3]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _params(sizes, seed=0):
    return [torch.nn.Parameter(R.make_p(n, seed + i, device="cuda")) for i, n in enumerate(sizes)]


def _set_grads(opt, params, seed, skip=()):
    for i, p in enumerate(params):
        wd = _group_of(opt, p)["weight_decay"] != 0
        p.grad = None if i in skip else R.make_g(p.numel(), seed + i, like_sign_of=p if wd else None, device="cuda").view_as(p)


def _group_of(opt, p):
    for g in opt.param_groups:
        if any(q is p for q in g["params"]):
            return g
    raise KeyError


def _cfg(group):
    return {k: group[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad")}


def _snapshot(opt, p):
    st = opt.state.get(p, {})
    z = torch.zeros_like(p)
    return dict(p=p.detach().clone(), m=st["exp_avg"].clone() if st else z, v=st["exp_avg_sq"].clone() if st else z,
                vmax=st["max_exp_avg_sq"].clone() if "max_exp_avg_sq" in st else z, t=int(st["step"].item()) if st else 0)


def _step_and_check(opt, params, label, worst=None, do_step=None):
    """One opt.step() over `params` (their .grad is set; None: the parameter sits out), every stepped tensor held to the bound
    against the restatement fed the state from BEFORE the step; the others bitwise unchanged.  -> the t each tensor was stepped with."""
    worst = {} if worst is None else worst
    before = [_snapshot(opt, p) for p in params]
    grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
    cfgs = [_cfg(_group_of(opt, p)) for p in params]
    (do_step or opt.step)()
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
        assert st["step"].item() == t and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32, label
        ref = R.step(b["p"], g, b["m"], b["v"], b["vmax"], t=t, **cfg)
        c, masks = R.achieved(ref, b, dict(p=p.detach(), m=st["exp_avg"], v=st["exp_avg_sq"], vmax=st.get("max_exp_avg_sq")))
        for k, val in c.items():
            worst[k] = max(worst.get(k, 0.0), val)
        assert masks and R.within_bound(c), (label, tuple(p.shape), t, c)
        ts.append(t)
    return ts


# ---- the per-step contract
def _build(config, params):
    from dvc_amd.optim import Adam
    if config == "train_py":
        return Adam(params, **TRAIN_PY)                                 # default eps, as train.py
    if config == "weight_decay":
        return Adam(params, lr=1e-3, weight_decay=1e-2)
    if config == "amsgrad":
        return Adam(params, lr=1e-3, amsgrad=True)
    assert config == "two_groups"
    return Adam([{"params": params[0::2]}, {"params": params[1::2], "lr": 4e-4}], **TRAIN_PY)


@pytest.mark.parametrize("config", ["train_py", "weight_decay", "amsgrad", "two_groups"])
def test_four_steps_meet_the_bound_at_every_size(config):
    params = _params(_sizes())
    opt = _build(config, params)
    worst = {}
    for it in range(1, 5):
        _set_grads(opt, params, 100 * it)
        assert _step_and_check(opt, params, (config, it), worst) == [it] * len(params)
    print(config, worst)
    if config == "two_groups":
        assert [_group_of(opt, p)["lr"] for p in params[:2]] == [2e-4, 4e-4]


def test_resumed_step_count():
    params = _params(_sizes(), seed=20)
    opt = _build("train_py", params)
    _set_grads(opt, params, 1)
    opt.step()
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.tensor(1000.0)
    opt.load_state_dict(sd)
    for it in (1, 2):
        _set_grads(opt, params, 10 + it)
        assert _step_and_check(opt, params, ("resumed", it)) == [1000 + it] * len(params)


def test_each_parameter_keeps_its_own_step():
    params = _params([5, _chunk() + 1, 7], seed=30)
    opt = _build("train_py", params)
    seen = []
    for it in range(1, 5):
        _set_grads(opt, params, 40 * it, skip=(1,) if it in (2, 3) else ())
        seen.append(_step_and_check(opt, params, ("own step", it)))
    assert seen == [[1, 1, 1], [2, None, 2], [3, None, 3], [4, 2, 4]]


# ---- misalignment, behind sentinels
SENTINEL = 12345.678


def _view(n, off, fill=None):
    """A view of n floats starting `off` elements into a sentinel-filled buffer (the buffer itself is 16-byte aligned)."""
    buf = torch.full((n + 8,), SENTINEL, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _sentinels_intact(buf, off, n):
    want = torch.full((1,), SENTINEL).view(torch.int32).item()
    bits = buf.view(torch.int32)
    return bool((bits[:off] == want).all()) and bool((bits[off + n:] == want).all())


@pytest.mark.parametrize("which", ["p", "g", "m", "v", "vmax"])
def test_misaligned_views_and_untouched_neighbours(which):
    """Each of the five pointers in turn starts 0 .. 4 elements into a buffer: offsets 1, 2, 3 take the scalar path, 0 and 4 the
    16-byte path with its scalar tail; the elements around the view keep their sentinel bits."""
    from dvc_amd import optim
    cases = [(n, off) for n in (6, _chunk() + 5) for off in (0, 1, 2, 3, 4)]
    bufs, params = [], []
    for i, (n, off) in enumerate(cases):
        if which == "p":
            buf, view = _view(n, off, R.make_p(n, 50 + i, device="cuda"))
            bufs.append(buf)
            params.append(torch.nn.Parameter(view))
            assert params[-1].data_ptr() == buf.data_ptr() + 4 * off
        else:
            params.append(torch.nn.Parameter(R.make_p(n, 50 + i, device="cuda")))
    opt = optim.Adam(params, lr=1e-3, amsgrad=True)
    _set_grads(opt, params, 60)
    _step_and_check(opt, params, (which, "first"))
    key = {"m": "exp_avg", "v": "exp_avg_sq", "vmax": "max_exp_avg_sq"}.get(which)
    if key:
        opt.load_state_dict(opt.state_dict())
        for p, (n, off) in zip(params, cases):
            buf, view = _view(n, off, opt.state[p][key])
            bufs.append(buf)
            opt.state[p][key] = view
    _set_grads(opt, params, 70)
    if which == "g":
        for p, (n, off) in zip(params, cases):
            buf, view = _view(n, off, p.grad)
            bufs.append(buf)
            p.grad = view
            assert p.grad.data_ptr() == buf.data_ptr() + 4 * off
    for p, (n, off) in zip(params, cases):
        ptrs = [p.data_ptr(), p.grad.data_ptr()] + [opt.state[p][k].data_ptr() for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")]
        assert optim.vector_path(*ptrs) == (off % 4 == 0), (which, n, off)
    assert _step_and_check(opt, params, (which, "second")) == [2] * len(cases)
    for buf, (n, off) in zip(bufs, cases):
        assert _sentinels_intact(buf, off, n), (which, n, off)


# ---- many tensors, one launch; independence; reproducibility
@contextlib.contextmanager
def _count_launches():
    from dvc_amd import ops
    calls, real = [], ops.adam_step

    def counted(tensor_table, n_tensors, chunk_table, n_chunks):
        calls.append((n_tensors, n_chunks))
        return real(tensor_table, n_tensors, chunk_table, n_chunks)

    ops.adam_step = counted
    try:
        yield calls
    finally:
        ops.adam_step = real


def _run_many(sizes, alone=None):
    """Two steps over tensors of `sizes` (or over tensor `alone` of them only, with the same values and gradients)."""
    from dvc_amd.optim import Adam
    params = _params(sizes, seed=80)
    grads = [[R.make_g(n, 1000 * it + i, device="cuda") for i, n in enumerate(sizes)] for it in (1, 2)]
    pick = range(len(sizes)) if alone is None else [alone]
    opt = Adam([params[i] for i in pick], weight_decay=0.0, **TRAIN_PY)
    for it in (0, 1):
        for i in pick:
            params[i].grad = grads[it][i]
        if alone is None and it == 1:
            _step_and_check(opt, params, ("many", it))
        else:
            opt.step()
    return {i: (params[i].detach(), opt.state[params[i]]["exp_avg"], opt.state[params[i]]["exp_avg_sq"]) for i in pick}


def test_many_tensors_in_one_launch_independent_and_reproducible():
    C = _chunk()
    sizes = [1] * 150 + [2 * C + 3] + [1] * 150
    with _count_launches() as calls:
        full = _run_many(sizes)
    assert calls == [(301, 300 + 3)] * 2                                   # one dvc_adam_step per step(), every tensor in it
    again = _run_many(sizes)
    for i in (0, 150, 300):
        with _count_launches() as calls:
            alone = _run_many(sizes, alone=i)
        assert calls == [(1, 3 if i == 150 else 1)] * 2
        for a, b, c in zip(full[i], alone[i], again[i]):
            assert _bits_equal(a, b) and _bits_equal(a, c), i


# ---- non-finite gradients
def test_non_finite_gradients_stay_in_their_elements():
    from dvc_amd.optim import Adam
    n = _chunk() + 5
    params = _params([n, n], seed=90)
    buf, view = _view(n, 1, params[1].detach())            # the second tensor on the scalar path
    params[1] = torch.nn.Parameter(view)
    opt = Adam(params, **TRAIN_PY)
    _set_grads(opt, params, 91)
    _step_and_check(opt, params, "finite first")
    _set_grads(opt, params, 92)
    bad = {3: float("nan"), 10: float("inf"), n - 1: float("-inf")}        # vector body, vector body, scalar tail
    for p in params:
        for i, val in bad.items():
            p.grad[i] = val
    _step_and_check(opt, params, "non-finite")          # same non-finite and NaN masks as the restatement, neighbours in bound
    for p in params:
        st = opt.state[p]
        for t in (p.detach(), st["exp_avg"], st["exp_avg_sq"]):
            assert sorted(torch.nonzero(~torch.isfinite(t)).flatten().tolist()) == sorted(bad)
        assert torch.isnan(p.detach()[[3, 10, n - 1]]).all() and torch.isnan(st["exp_avg"][3]) and torch.isinf(st["exp_avg_sq"][10])
    assert _sentinels_intact(buf, 1, n)


# ---- zero_grad, streams, autograd's version counter, capture
@pytest.mark.parametrize("set_to_none", [True, False])
def test_steps_across_zero_grad(set_to_none):
    params = _params([7, _chunk() + 1], seed=110)
    opt = _build("train_py", params)
    for it in range(1, 4):
        coef = [R.make_g(p.numel(), 120 * it + i, device="cuda") for i, p in enumerate(params)]
        sum((p * c).sum() for p, c in zip(params, coef)).backward()
        for p, c in zip(params, coef):
            assert torch.equal(p.grad, c)
        assert _step_and_check(opt, params, ("zero_grad", set_to_none, it)) == [it, it]
        opt.zero_grad(set_to_none=set_to_none)
        assert all((p.grad is None) if set_to_none else bool((p.grad == 0).all()) for p in params)


def test_step_on_a_side_stream():
    params = _params([5, 2 * _chunk() + 3], seed=130)
    opt = _build("train_py", params)
    side = torch.cuda.Stream()

    def on_the_side_stream():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            opt.step()
        side.synchronize()

    for it in (1, 2, 3):                    # (both staging buffers, and the first one again)
        _set_grads(opt, params, 131 * it)
        assert _step_and_check(opt, params, ("side stream", it), do_step=on_the_side_stream) == [it, it]
    _set_grads(opt, params, 132)
    assert _step_and_check(opt, params, "back on the default stream") == [4, 4]


@pytest.mark.parametrize("which", ["dvc", "torch"])
def test_stale_graph_refuses_its_backward(which):
    from dvc_amd.optim import Adam
    p = torch.nn.Parameter(R.make_p(9, 140, device="cuda"))
    opt = (Adam if which == "dvc" else torch.optim.Adam)([p], lr=1e-3)
    y = (p * p).sum()
    p.grad = torch.ones_like(p)
    version = p._version
    opt.step()
    assert p._version > version
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()


def test_step_refuses_stream_capture_before_any_launch():
    params = _params([5, _chunk() + 1], seed=150)
    opt = _build("train_py", params)
    _set_grads(opt, params, 151)
    opt.step()
    torch.cuda.synchronize()
    before = [_snapshot(opt, p) for p in params]
    graph, other = torch.cuda.CUDAGraph(), torch.zeros(8, device="cuda")
    with _count_launches() as calls:
        with torch.cuda.graph(graph):
            other.add_(1.0)                 # (an ordinary captured kernel: the capture itself is a normal one)
            with pytest.raises(RuntimeError, match="cannot be captured into a graph"):
                opt.step()
    torch.cuda.synchronize()
    assert calls == []
    for p, b in zip(params, before):
        st = opt.state[p]
        assert _bits_equal(p.detach(), b["p"]) and _bits_equal(st["exp_avg"], b["m"]) and st["step"].item() == 1
    assert _step_and_check(opt, params, "after the refused capture") == [2, 2]


def test_step_refusals_on_the_device():
    from dvc_amd.optim import Adam
    p = torch.nn.Parameter(torch.ones(4, 6, device="cuda").t())
    p.grad = torch.ones(6, 4, device="cuda")
    with pytest.raises(ValueError, match="not contiguous"):
        Adam([p]).step()
    h = torch.nn.Parameter(torch.ones(4, device="cuda", dtype=torch.float16))
    h.grad = torch.ones_like(h)
    with pytest.raises(TypeError, match="float32"):
        Adam([h]).step()
    q = torch.nn.Parameter(R.make_p(24, 160, device="cuda").view(4, 6))
    opt = Adam([q], **TRAIN_PY)
    q.grad = R.make_g(24, 161, device="cuda").view(6, 4).t()              # a non-contiguous gradient is made contiguous
    assert not q.grad.is_contiguous()
    _step_and_check(opt, [q], "transposed gradient")
    opt.state[q]["exp_avg"] = opt.state[q]["exp_avg"].double()
    with pytest.raises(TypeError, match="exp_avg"):
        opt.step()
    assert opt.state[q]["step"].item() == 1                                  # a refused step advances nothing
    c = torch.nn.Parameter(torch.ones(3))
    c.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Adam([q, c]).step()


# ---- interchange with torch.optim.Adam on the device; schedulers
@pytest.mark.parametrize("amsgrad", [False, True])
def test_state_dict_interchange_on_the_device(amsgrad):
    from dvc_amd.optim import Adam
    params = _params([7, _chunk() + 1], seed=170)
    topt = torch.optim.Adam(params, amsgrad=amsgrad, **TRAIN_PY)
    for it in range(1, 4):
        _set_grads(topt, params, 171 * it)
        topt.step()
    opt = Adam(params, lr=1.0)
    opt.load_state_dict(topt.state_dict())
    assert opt.param_groups[0]["lr"] == 2e-4 and opt.param_groups[0]["betas"] == (0.5, 0.999)
    _set_grads(opt, params, 999)
    assert _step_and_check(opt, params, "fourth step on torch's state") == [4, 4]
    back = torch.optim.Adam(params, lr=1.0)
    back.load_state_dict(opt.state_dict())
    _set_grads(back, params, 1001)
    back.step()
    assert all(back.state[p]["step"].item() == 5 and bool(torch.isfinite(p).all()) for p in params)


def test_step_lr_scheduler():
    params = _params([7, _chunk() + 1], seed=180)
    opt = _build("train_py", params)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    lrs = []
    for it in range(1, 5):
        _set_grads(opt, params, 181 * it)
        lrs.append(opt.param_groups[0]["lr"])
        _step_and_check(opt, params, ("StepLR", it))          # the restatement's lr is the group's, read before the step
        sched.step()
    assert lrs == [2e-4, 2e-4, 1e-4, 1e-4]


# ---- through a real network
def test_two_training_iterations_of_colorvidnet():
    from dvc_amd import synth
    from dvc_amd.optim import Adam
    from models.ColorVidNet import ColorVidNet
    with contextlib.redirect_stdout(io.StringIO()):
        net = ColorVidNet(7)
    net.load_state_dict(synth.colorvidnet_state_dict(0, contractive=True))
    net = net.cuda().train()
    params = list(net.parameters())
    assert len(params) == 65
    opt = Adam(params, **TRAIN_PY)
    gen = torch.Generator().manual_seed(190)
    x = ((torch.rand(1, 7, 16, 24, generator=gen) * 2 - 1) * 50).cuda()
    outs = []
    for it in (1, 2):
        opt.zero_grad(set_to_none=True)
        ab = net(x)
        outs.append(ab.detach().clone())
        (ab * ab).sum().backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
        with _count_launches() as calls:
            assert _step_and_check(opt, params, ("ColorVidNet", it)) == [it] * 65
        assert len(calls) == 1 and calls[0][0] == 65
    assert not torch.equal(outs[0], outs[1])                # the second forward ran on the updated weights
