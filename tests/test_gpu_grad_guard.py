"""GPU: the gradient guard — dvc_grad_norm, dvc_adam_advance_guarded, dvc_adam_step_guarded, dvc_grad_scale (csrc/optim.hip) and
dvc_amd.optim.GuardedAdam / grad_norm / clip_grad_norm_ on top of them.  Exact norms on integer data, bit for bit against an int64
sum; the reduction's two strides, its independence of the table, of repetition and of alignment; random gradients at three scales
within the bounds derived in tests/grad_guard_reference.py; the overflow case; whole-step skips on a NaN or Inf wherever it sits;
GuardedAdam without options bit-identical to CapturableAdam; clipping held to tests/adam_reference.py's bound on the device's own
coefficient; the stand-alone clip_grad_norm_; sentinels around every gradient; and a captured step replayed through a skipped
step, bit for bit against eager steps.

Sizes 1, 3, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 5 plus one tensor that is a view 1 element into a buffer (the dword path):
the sizes of tests/test_gpu_capturable_adam.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as A  # noqa: E402
import grad_guard_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096
SIZES = [1, 3, C - 1, C, C + 1, 2 * C + 5]
VIEW_N = 4097
FLT_MAX = float(np.finfo(np.float32).max)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _view_into(values, offset=1, fill=12345.678):
    """`values` copied `offset` elements into a `fill`ed buffer -> (the view, the buffer)."""
    n = values.numel()
    buf = torch.full((n + 8,), fill, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n]
    view.copy_(values)
    return view, buf


def _int_grads(seed):
    """Integers in +-2^11 over the six sizes and the misaligned view."""
    gen = torch.Generator().manual_seed(seed)
    grads = [torch.randint(-2048, 2049, (n,), generator=gen).float().cuda() for n in SIZES]
    grads.append(_view_into(torch.randint(-2048, 2049, (VIEW_N,), generator=gen).float().cuda())[0])
    return grads


def _int_sumsq(grads):
    return float(sum(int((g.long() ** 2).sum().item()) for g in grads))


def _run_norm(grads, max_norm=math.inf, keep_nonfinite=False, guard=None):
    """dvc_grad_norm on the tables of `grads` -> (record as a dict, partials as a float64 CPU tensor, (table, n_t, chunks, n_c, guard))."""
    from dvc_amd import ops, optim
    tensors, chunks = optim.build_norm_tables(grads)
    table = torch.from_numpy(np.concatenate([tensors.view(np.uint8), chunks.view(np.uint8)])).cuda()
    partials = torch.full((len(chunks),), -1.0, dtype=torch.float64, device="cuda")
    guard = optim.new_guard("cuda") if guard is None else guard
    ops.grad_norm(table, len(tensors), table[tensors.nbytes:], len(chunks), partials, max_norm, guard, keep_nonfinite=keep_nonfinite)
    return optim.read_guard(guard), partials.cpu(), (table, len(tensors), table[tensors.nbytes:], len(chunks), guard)


def _f32(x):
    return float(np.float32(x))


def _check_exact(rec, s):
    assert rec["sumsq"] == s and rec["total_norm"] == _f32(math.sqrt(s)) and rec["found_inf"] == 0 and rec["skipped"] == 0, (rec, s)


# ---- exact norms
def test_exact_norms():
    rec, partials, _ = _run_norm([torch.tensor([3.0, 4.0], device="cuda")])
    assert rec == dict(total_norm=5.0, clip_coef=1.0, found_inf=0, skipped=0, sumsq=25.0) and partials.tolist() == [25.0]
    rec, partials, _ = _run_norm([torch.ones(16384, device="cuda")])
    assert rec["total_norm"] == 128.0 and rec["sumsq"] == 16384.0 and partials.tolist() == [4096.0] * 4
    rec, _, _ = _run_norm([torch.zeros(n, device="cuda") for n in SIZES], max_norm=0.5)
    assert rec == dict(total_norm=0.0, clip_coef=1.0, found_inf=0, skipped=0, sumsq=0.0)
    grads = _int_grads(1)
    for g in grads:                                 # every size alone
        _check_exact(_run_norm([g])[0], _int_sumsq([g]))
    _check_exact(_run_norm(grads)[0], _int_sumsq(grads))


# ---- reduction paths and determinism
def test_both_strides_table_independence_repeats_and_alignment():
    gen = torch.Generator().manual_seed(2)
    flat = torch.randint(-2048, 2049, (2100,), generator=gen).float().cuda()
    ones = [flat[i:i + 1] for i in range(2100)]                 # one-element tensors at every 4-byte alignment
    for count in (300, 2100):                                   # past stage 2's 256 threads; past stage 1's 2,048 workgroups
        rec, partials, _ = _run_norm(ones[:count])
        _check_exact(rec, _int_sumsq(ones[:count]))
        assert torch.equal(partials, flat[:count].cpu().double() ** 2)
    # one tensor alone and inside the 300-tensor table: the same partials, bit for bit
    gen = torch.Generator().manual_seed(3)
    big = (torch.randn(2 * C + 5, generator=gen) * 3.7).cuda()
    alone_rec, alone, _ = _run_norm([big])
    _, inside, _ = _run_norm(ones[:150] + [big] + ones[150:299])
    assert torch.equal(alone.view(torch.int64), inside[150:153].view(torch.int64))
    # a repeat is bit-identical
    again_rec, again, _ = _run_norm([big])
    assert again_rec == alone_rec and torch.equal(alone.view(torch.int64), again.view(torch.int64))
    # aligned and one-element-misaligned copies of the same data
    shifted, _ = _view_into(big)
    assert big.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    shifted_rec, shifted_partials, _ = _run_norm([shifted])
    assert shifted_rec == alone_rec and torch.equal(alone.view(torch.int64), shifted_partials.view(torch.int64))


# ---- random gradients
def _random_grads(seed, scale):
    gen = torch.Generator().manual_seed(seed)
    grads = [(torch.randn(n, generator=gen, dtype=torch.float64) * scale).float().cuda() for n in SIZES]
    grads.append(_view_into((torch.randn(VIEW_N, generator=gen, dtype=torch.float64) * scale).float().cuda())[0])
    return grads


def _check_against_restatement(rec, grads, max_norm):
    n = sum(g.numel() for g in grads)
    s, norm = R.sumsq(grads), R.norm(grads)
    assert abs(rec["sumsq"] - s) <= n * R.U * s, (rec, s)
    assert abs(rec["total_norm"] - norm) <= R.norm_bound(n) * norm, (rec, norm)
    want = _f32(R.coefficient(norm, max_norm))
    print(f"n {n}: total_norm off by {abs(rec['total_norm'] - norm) / norm / R.E:.3f} e (bound {R.norm_bound(n) / R.E:.5f} e), "
          f"clip_coef {rec['clip_coef']!r} against {want!r}")
    assert R.ulps(rec["clip_coef"], want) <= 1, (rec, want)
    assert rec["found_inf"] == 0


@pytest.mark.parametrize("scale", [1e-20, 1.0, 1e18])
def test_random_gradients_within_the_derived_bounds(scale):
    grads = _random_grads(4, scale)
    for max_norm in (0.37 * scale, 1e6 * scale):               # far below the norm, and far above it
        rec, _, _ = _run_norm(grads, max_norm=max_norm)
        _check_against_restatement(rec, grads, max_norm)
    assert _run_norm(grads)[0]["clip_coef"] == 1.0             # max_norm = +inf: exactly 1


def test_norm_past_the_fp32_range_is_not_a_skip():
    g = torch.zeros(C + 1, device="cuda")
    g[[0, 1, C - 1, C]] = torch.tensor([FLT_MAX, -FLT_MAX, FLT_MAX, FLT_MAX], device="cuda")
    rec, _, _ = _run_norm([g], max_norm=1.0)
    assert rec["total_norm"] == math.inf and rec["found_inf"] == 0 and rec["skipped"] == 0 and rec["sumsq"] == 4.0 * FLT_MAX ** 2
    want = _f32(R.coefficient(2.0 * FLT_MAX, 1.0))
    assert 0.0 < rec["clip_coef"] < 1e-38 and math.isfinite(rec["clip_coef"])
    assert abs(int(np.float32(rec["clip_coef"]).view(np.int32)) - int(np.float32(want).view(np.int32))) <= 1, (rec, want)      # (a subnormal: ulps by bits)


# ---- non-finite gradients
def _params(seed=0):
    """The six sizes, then the view: -> (parameters, the view's sentinel-filled buffer)."""
    params = [torch.nn.Parameter(A.make_p(n, seed + i, device="cuda")) for i, n in enumerate(SIZES)]
    view, buf = _view_into(A.make_p(VIEW_N, seed + 50, device="cuda"))
    params.append(torch.nn.Parameter(view))
    assert params[-1].data_ptr() == buf.data_ptr() + 4
    return params, buf


def _clones(params):
    return [torch.nn.Parameter(p.detach().clone()) for p in params]


def _make_grads(params, seed, wd=False):
    """adam_reference.make_g per tensor; the one-element tensors past the seven standard ones (all positive) share one draw."""
    extra = torch.rand(len(params), generator=torch.Generator().manual_seed(seed)).cuda() + 0.5
    return [extra[i:i + 1].clone() if i >= 7 else A.make_g(p.numel(), seed + i, like_sign_of=p if wd else None, device="cuda").view_as(p)
            for i, p in enumerate(params)]


def _all_bytes(opt, params):
    out = []
    for p in params:
        st = opt.state[p]
        out += [p.detach().clone(), p.grad.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone().reshape(1)]
        if "max_exp_avg_sq" in st:
            out.append(st["max_exp_avg_sq"].clone())
    return out


def _same_state(params, opt, twins, ref):
    for p, q in zip(params, twins):
        a, b = opt.state[p], ref.state[q]
        assert _bits_equal(p.detach(), q.detach()) and _bits_equal(a["exp_avg"], b["exp_avg"]) and _bits_equal(a["exp_avg_sq"], b["exp_avg_sq"])
        if "max_exp_avg_sq" in b:
            assert _bits_equal(a["max_exp_avg_sq"], b["max_exp_avg_sq"])
        assert a["step"].item() == b["step"].item()


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize("where", ["first", "tail_last", "view", "last_of_2100"])
def test_a_nonfinite_gradient_skips_the_whole_step(where, bad):
    from dvc_amd import optim
    params, _ = _params(seed=300)
    if where == "last_of_2100":
        params = params[:3] + [torch.nn.Parameter(torch.full((1,), 0.5, device="cuda")) for _ in range(2100 - 3)]
    twins = _clones(params)
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-2, amsgrad=True)
    opt, ref = optim.GuardedAdam(params, **kw), optim.GuardedAdam(twins, **kw)
    steps = [_make_grads(params, 100 * it, wd=True) for it in (1, 2, 3)]
    for p, q, g in zip(params, twins, steps[0]):
        p.grad, q.grad = g.clone(), g.clone()
    opt.step()
    ref.step()
    for p, g in zip(params, steps[1]):
        p.grad.copy_(g)
    target = {"first": (0, 0), "tail_last": (5, 2 * C + 4), "view": (6, 2000), "last_of_2100": (len(params) - 1, 0)}[where]
    if where == "view":
        p = params[6]
        g, _ = _view_into(p.grad.clone())
        p.grad = g.view_as(p)
        assert p.grad.data_ptr() % 16 == 4
    params[target[0]].grad.view(-1)[target[1]] = bad
    before = _all_bytes(opt, params)
    skipped0 = opt.skipped_steps.item()
    opt.step()
    assert optim.read_guard(opt._dvc_guard)["found_inf"] == 1
    assert opt.skipped_steps.item() == skipped0 + 1 == 1 and not math.isfinite(opt.last_grad_norm.item())
    for a, b in zip(before, _all_bytes(opt, params)):
        assert _bits_equal(a, b)
    assert all(opt.state[p]["step"].item() == 1 for p in params)
    # the next step with finite gradients goes on from step + 1, exactly as if the bad one had never come
    for p, q, g in zip(params, twins, steps[2]):
        p.grad.copy_(g)
        q.grad.copy_(g)
    opt.step()
    ref.step()
    assert opt.skipped_steps.item() == 1 and ref.skipped_steps.item() == 0 and math.isfinite(opt.last_grad_norm.item())
    assert all(opt.state[p]["step"].item() == 2 for p in params)
    _same_state(params, opt, twins, ref)


def test_skip_nonfinite_off_behaves_like_capturable_adam():
    from dvc_amd import optim
    params, _ = _params(seed=310)
    twins = _clones(params)
    opt, ref = optim.GuardedAdam(params, lr=2e-4, skip_nonfinite=False), optim.CapturableAdam(twins, lr=2e-4)
    for it in (1, 2):
        for p, q, g in zip(params, twins, _make_grads(params, 100 * it)):
            if it == 2:
                g.view(-1)[0] = math.nan
            p.grad, q.grad = g, g.clone()
        opt.step()
        ref.step()
    rec = optim.read_guard(opt._dvc_guard)
    assert rec["found_inf"] == 0 and rec["skipped"] == 0 and rec["clip_coef"] == 1.0 and math.isnan(rec["total_norm"])
    assert all(opt.state[p]["step"].item() == 2 and bool(torch.isnan(p.detach().view(-1)[0])) for p in params)
    _same_state(params, opt, twins, ref)


# ---- no options: CapturableAdam's bits
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_without_clipping_three_steps_equal_capturable_adam(weight_decay, amsgrad):
    from dvc_amd import optim
    params, _ = _params(seed=320)
    twins = _clones(params)
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=weight_decay, amsgrad=amsgrad)
    opt = optim.GuardedAdam([{"params": params[0::2]}, {"params": params[1::2], "lr": 4e-4}], max_grad_norm=None, **kw)
    ref = optim.CapturableAdam([{"params": twins[0::2]}, {"params": twins[1::2], "lr": 4e-4}], **kw)
    for it in (1, 2, 3):
        grads = _make_grads(params, 100 * it, wd=weight_decay != 0)
        for p, q, g in zip(params, twins, grads):
            p.grad, q.grad = g, g.clone()
        opt.step()
        ref.step()
        rec = optim.read_guard(opt._dvc_guard)
        assert rec["clip_coef"] == 1.0 and rec["found_inf"] == 0
        assert abs(rec["total_norm"] - R.norm(grads)) <= R.norm_bound(sum(g.numel() for g in grads)) * R.norm(grads)
    assert all(opt.state[p]["step"].item() == 3 for p in params)
    _same_state(params, opt, twins, ref)


# ---- clipping active
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_clipped_steps_meet_the_adam_bound_and_leave_grad_alone(weight_decay, amsgrad):
    from dvc_amd import optim
    params, _ = _params(seed=330)
    cfg = dict(lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=weight_decay, amsgrad=amsgrad)
    opt = optim.GuardedAdam(params, **cfg)
    worst = {}
    for it in (1, 2, 3):
        grads = _make_grads(params, 100 * it, wd=weight_decay != 0)
        measured = R.norm(grads)
        opt.max_grad_norm = 0.5 * measured                      # half the norm: every step is clipped by about 0.5
        for p, g in zip(params, grads):
            p.grad = g.clone()
        states = []
        for p in params:
            st, z = opt.state.get(p, {}), torch.zeros_like(p)
            states.append(dict(p=p.detach().clone(), m=st["exp_avg"].clone() if st else z, v=st["exp_avg_sq"].clone() if st else z,
                               vmax=st["max_exp_avg_sq"].clone() if "max_exp_avg_sq" in st else z, t=it - 1))
        opt.step()
        rec = optim.read_guard(opt._dvc_guard)
        assert R.ulps(rec["clip_coef"], _f32(R.coefficient(measured, 0.5 * measured))) <= 1 and 0.49 < rec["clip_coef"] < 0.51
        _, refs, info = R.guarded_step(states, grads, [cfg] * len(params), max_norm=0.5 * measured, coef=rec["clip_coef"])
        assert info["found_inf"] == 0
        for p, g, b, ref in zip(params, grads, states, refs):
            st = opt.state[p]
            assert _bits_equal(p.grad, g) and st["step"].item() == it
            c, masks = A.achieved(ref, b, dict(p=p.detach(), m=st["exp_avg"], v=st["exp_avg_sq"], vmax=st.get("max_exp_avg_sq")))
            for k, val in c.items():
                worst[k] = max(worst.get(k, 0.0), val)
            assert masks and A.within_bound(c), (it, tuple(p.shape), c)
    print(weight_decay, amsgrad, worst)


# ---- the stand-alone functions
def test_clip_grad_norm_function():
    from dvc_amd import optim
    params, buf = _params(seed=340)
    grads = _random_grads(5, 1.0)
    for p, g in zip(params, grads):
        p.grad = g.clone().view_as(p)
    n, norm = sum(g.numel() for g in grads), R.norm(grads)
    got = optim.grad_norm(params)
    assert got.shape == () and got.dtype == torch.float32 and got.is_cuda and abs(got.item() - norm) <= R.norm_bound(n) * norm
    # a norm below max_norm leaves the gradients bit-identical
    out = optim.clip_grad_norm_(params, 2.0 * norm)
    assert out.shape == () and out.is_cuda and abs(out.item() - norm) <= R.norm_bound(n) * norm
    assert all(_bits_equal(p.grad.view(-1), g) for p, g in zip(params, grads))
    # above it: the restatement's coefficient to 1 ulp, and fl32(c g) for one of the (at most two) candidate coefficients
    out = optim.clip_grad_norm_(params, 0.25 * norm, norm_type=2, foreach=True)
    assert abs(out.item() - norm) <= R.norm_bound(n) * norm
    want = np.float32(R.coefficient(norm, 0.25 * norm))
    cands = [want, np.nextafter(want, np.float32(0)), np.nextafter(want, np.float32(1))]
    assert any(all(_bits_equal(p.grad.view(-1), R.clipped(g, float(c))) for p, g in zip(params, grads)) for c in cands)
    assert abs(R.norm([p.grad for p in params]) - 0.25 * norm) <= 1e-6 * norm
    # non-finite: the error on request, torch's scaling otherwise
    params[2].grad.view(-1)[7] = math.nan
    kept = [p.grad.clone() for p in params]
    with pytest.raises(RuntimeError, match="non-finite, so it cannot be clipped"):
        optim.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
    assert all(_bits_equal(p.grad, k) for p, k in zip(params, kept))
    assert math.isnan(optim.clip_grad_norm_(params, 1.0).item()) and all(bool(torch.isnan(p.grad).all()) for p in params)
    # and it refuses a capture
    for p, g in zip(params, grads):
        p.grad.copy_(g.view_as(p))
    torch.cuda.synchronize()
    graph, other = torch.cuda.CUDAGraph(), torch.zeros(8, device="cuda")
    with torch.cuda.graph(graph):
        other.add_(1.0)
        with pytest.raises(RuntimeError, match="cannot be captured into a graph"):
            optim.grad_norm(params)
        with pytest.raises(RuntimeError, match="cannot be captured into a graph"):
            optim.clip_grad_norm_(params, 1.0)
    torch.cuda.synchronize()
    assert all(_bits_equal(p.grad.view(-1), g) for p, g in zip(params, grads))


# ---- sentinels
def test_nothing_outside_a_gradient_is_read_or_written():
    """Every size at offsets 0 .. 4 elements into a buffer of +Inf: one Inf read would make the sum non-finite; dvc_grad_scale
    (coefficient 0.5: exact on integers) must leave every sentinel bit alone."""
    from dvc_amd import ops
    gen = torch.Generator().manual_seed(6)
    grads, bufs, origs = [], [], []
    for n in SIZES:
        for off in range(5):
            v = torch.randint(-2048, 2049, (n,), generator=gen).float().cuda()
            g, buf = _view_into(v, offset=off, fill=math.inf)
            grads.append(g), bufs.append((buf, off, n)), origs.append(v)
    s = _int_sumsq(origs)
    rec, _, (table, n_t, chunks, n_c, guard) = _run_norm(grads, max_norm=0.5 * math.sqrt(s) + 0.5e-6)       # 0.5 (norm + 1e-6)
    _check_exact(rec, s)
    assert rec["clip_coef"] == 0.5
    ops.grad_scale(table, n_t, chunks, n_c, guard)
    for (buf, off, n), v in zip(bufs, origs):
        assert bool(torch.isposinf(buf[:off]).all()) and bool(torch.isposinf(buf[off + n:]).all())
        assert _bits_equal(buf[off:off + n], v * 0.5)


# ---- graphs
@pytest.mark.parametrize("upload_captured", [False, True])
def test_captured_guarded_step_replays_through_a_skipped_step(upload_captured):
    """One eager step, one step() captured, three replays with the static gradients rewritten in place and a NaN planted before the
    second; against the same three eager steps on clones.  upload_captured: the captured step is the first of an optimiser that
    loaded the warmed-up state, so the table upload is a node of the graph."""
    from dvc_amd import optim
    params, _ = _params(seed=350)
    twins = _clones(params)
    grads = [_make_grads(params, 500 * it, wd=True) for it in (1, 2, 3, 4)]
    grads[2][4].view(-1)[C] = math.nan
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-2, amsgrad=True, max_grad_norm=0.5 * R.norm(grads[0]))
    ref = optim.GuardedAdam(twins, **kw)
    for step in grads:
        for q, g in zip(twins, step):
            q.grad = g.clone()
        ref.step()
    assert ref.skipped_steps.item() == 1 and all(ref.state[q]["step"].item() == 3 for q in twins)

    opt = optim.GuardedAdam(params, **kw)
    static = [g.clone() for g in grads[0]]
    for p, s in zip(params, static):
        p.grad = s
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                      # the eager step: creates the state
    side.synchronize()
    if upload_captured:
        fresh = optim.GuardedAdam(params, **kw)
        fresh.load_state_dict(opt.state_dict())
        opt = fresh
    torch.cuda.synchronize()
    calls, real = [], (optim.CapturableAdam._upload, optim.ops.grad_norm, optim.ops.adam_advance_guarded, optim.ops.adam_step_guarded)
    try:
        optim.CapturableAdam._upload = lambda self, *a: (calls.append("upload"), real[0](self, *a))[1]
        optim.ops.grad_norm = lambda *a, **k: (calls.append("norm"), real[1](*a, **k))[1]
        optim.ops.adam_advance_guarded = lambda *a: (calls.append("advance"), real[2](*a))[1]
        optim.ops.adam_step_guarded = lambda *a: (calls.append("step"), real[3](*a))[1]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step()
    finally:
        optim.CapturableAdam._upload, optim.ops.grad_norm, optim.ops.adam_advance_guarded, optim.ops.adam_step_guarded = real
    assert calls == (["upload"] if upload_captured else []) + ["norm", "advance", "step"]
    assert opt._dvc_resident.captured and opt._dvc_resident.guard is opt._dvc_guard
    torch.cuda.synchronize()
    assert all(opt.state[p]["step"].item() == 1 for p in params) and opt.skipped_steps.item() == 0       # a capture runs nothing
    norms = []
    for it in (1, 2, 3):
        for s, g in zip(static, grads[it]):
            s.copy_(g)
        graph.replay()
        opt.mark_updated()
        norms.append(opt.last_grad_norm.item())
    torch.cuda.synchronize()
    assert all(opt.state[p]["step"].item() == 3 for p in params) and opt.skipped_steps.item() == 1
    assert math.isfinite(norms[0]) and math.isnan(norms[1]) and math.isfinite(norms[2])
    _same_state(params, opt, twins, ref)
    assert _bits_equal(opt._dvc_guard.view(torch.int32), ref._dvc_guard.view(torch.int32))
