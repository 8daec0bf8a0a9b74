"""GPU: dvc_amd.losses / dvc_loss_fwd, dvc_loss_bwd (csrc/loss.hip) held to the float64 restatement tests/losses_reference.py at the
bounds derived there (|value - value64| <= 6 * 2^-24 * A, |dx - dx64| <= 6 * 2^-24 * |dx64|, no absolute terms) — over sizes around
the wave, the workgroup and the chunk, both load paths, every weight layout, tensor and scalar targets — and, bit for bit: a term
alone against the same term in any fused table, repeated calls, target.grad == -input.grad.  Then non-finite inputs, the launch
count, the capture refusal, a side stream, and ColorVidNet's 65 parameter gradients under a fused two-term loss."""
import contextlib
import io
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096        # DVC_LOSS_CHUNK == dvc_amd.losses.CHUNK (test_one_forward_and_one_backward_call_whatever_the_terms asserts it)
SIZES = [1, 3, 63, 64, 65, 255, 257, C - 1, C, C + 1, 2 * C + 1]
MASKED = [((3, 2, 1, 5), (3, 1, 1, 5)),         # odd plane: the broadcast weight is read element by element
          ((2, 3, 2, 4), (2, 1, 2, 4)),         # plane % 4 == 0: 16-byte loads of the broadcast weight
          ((2, 2, 8, 520), (2, 1, 8, 520)),     # plane 4160: the broadcast crosses chunk boundaries mid-image
          ((2, 2, 8, 520), (2, 2, 8, 520))]     # weights of the input's shape
HELPERS = {"mse": ("mse_loss", "weighted_mse_loss"), "l1": ("l1_loss", "weighted_l1_loss")}


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _helper(kind, x, t, w):
    from dvc_amd import losses
    plain, weighted = HELPERS[kind]
    return getattr(losses, plain)(x, t) if w is None else getattr(losses, weighted)(x, t, w)


def _misaligned(v):
    """The same values in a contiguous tensor whose storage starts one element (4 bytes) past a 16-byte boundary."""
    buf = torch.empty(v.numel() + 1, device=v.device)
    out = buf[1:].view(v.shape)
    out.copy_(v)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _check_term(kind, x, t, w, label):
    """Value and gradients of one helper call against the restatement; x requires grad, and t if it is a tensor."""
    x = x.detach().requires_grad_(True)
    tt = t.detach().requires_grad_(True) if isinstance(t, torch.Tensor) else t
    loss = _helper(kind, x, tt, w)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    (3 * loss).backward()
    ref = R.term(kind, x, t, w, upstream=3.0)
    ev, eg = R.value_error(loss.item(), ref), R.grad_error(x.grad, ref)
    print(label, "value error / (EPS A) =", ev, " grad error / (EPS |dx64|) =", eg)
    assert ev <= R.C_VALUE, (label, ev)
    assert eg <= R.C_GRAD, (label, eg)
    assert x.grad.shape == x.shape
    if isinstance(t, torch.Tensor):
        assert _bits_equal(tt.grad, -x.grad), label
    return loss.detach(), x.grad


# ---- values and gradients against float64
@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_paths_and_targets(kind, n):
    x, t, _ = R.make_case((n,), 1000 + n, device="cuda")
    if n > 2:
        x[n // 2] = t[n // 2]           # planted: x == t, the gradient there is exactly 0 (grad_error demands it)
    assert x.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0        # the 16-byte path ...
    v_al, g_al = _check_term(kind, x, t, None, (kind, n, "aligned, tensor target"))
    if n > 2:
        assert g_al[n // 2].item() == 0.0
    for xm, tm, label in ((_misaligned(x), t, "x misaligned"), (x, _misaligned(t), "t misaligned")):     # ... and the scalar one
        v, g = _check_term(kind, xm, tm, None, (kind, n, label))
        assert _bits_equal(v, v_al) and _bits_equal(g, g_al)        # the path changes the loads, not the order of the sum
    for scalar in (0, 0.5):
        if n > 2:
            x[n // 2] = scalar
        _check_term(kind, x, scalar, None, (kind, n, "scalar target", scalar))
        _check_term(kind, _misaligned(x), scalar, None, (kind, n, "scalar target, misaligned", scalar))
    # default target: the reference's `target=0`
    from dvc_amd import losses
    plain = getattr(losses, HELPERS[kind][0])
    if n > 2:
        x[n // 2] = 0.0
    assert _bits_equal(plain(x), plain(x, 0))


@pytest.mark.parametrize("kind", ["mse", "l1"])
@pytest.mark.parametrize("shape,mask", MASKED)
@pytest.mark.parametrize("signed", [False, True])
def test_weight_layouts(kind, shape, mask, signed):
    x, t, w = R.make_case(shape, 2000 + sum(shape) + len(mask) * signed, mask, signed, device="cuda")
    x.view(-1)[x.numel() // 3] = t.view(-1)[x.numel() // 3]
    v, g = _check_term(kind, x, t, w, (kind, shape, mask, signed))
    vm, gm = _check_term(kind, _misaligned(x), t, _misaligned(w), (kind, shape, mask, signed, "misaligned"))
    assert _bits_equal(v, vm) and _bits_equal(g, gm)
    _check_term(kind, x, 0.5, w, (kind, shape, mask, signed, "scalar target"))
    if not signed:
        assert bool((g[w.expand_as(x) == 0] == 0).all())        # nothing flows where the mask is 0


def test_only_the_side_that_requires_grad_gets_one():
    from dvc_amd import losses
    x, t, w = R.make_case((2, 3, 2, 4), 7, (2, 1, 2, 4), device="cuda")
    tt = t.clone().requires_grad_(True)
    loss = losses.weighted_l1_loss(x, tt, w)            # train.py puts the detached side in either position
    (3 * loss).backward()
    assert x.grad is None and not x.requires_grad
    ref = R.term("l1", x, t, w, upstream=3.0)
    ref["dx64"] = -ref["dx64"]
    assert R.grad_error(tt.grad, ref) <= R.C_GRAD
    with torch.no_grad():
        assert not losses.mse_loss(x.requires_grad_(True)).requires_grad
    assert not losses.mse_loss(x.detach(), t).requires_grad


def test_l1_gradient_has_one_magnitude():
    from dvc_amd import losses
    for n in (65, 2 * C + 1):
        x, t, _ = R.make_case((n,), 31 + n, device="cuda")
        x[5] = t[5]
        x.requires_grad_(True)
        (3 * losses.l1_loss(x, t)).backward()
        mags = x.grad.abs()[x.grad != 0].view(torch.int32)
        assert x.grad[5].item() == 0 and mags.numel() == n - 1 and bool((mags == mags[0]).all())
        assert torch.equal(torch.sign(x.grad), torch.sign(x.detach() - t))


def test_non_contiguous_inputs_take_torchs_adjoint():
    from dvc_amd import losses
    base = torch.randn(6, 5, device="cuda", requires_grad=True)
    t = torch.randn(5, 6, device="cuda")
    (3 * losses.mse_loss(base.t(), t)).backward()
    ref = R.term("mse", base.detach().t().contiguous(), t, upstream=3.0)
    assert base.grad.shape == (6, 5) and R.grad_error(base.grad.t().contiguous(), ref) <= R.C_GRAD


# ---- fused
def _five_terms(seed=50):
    """Sizes 1, 65, 4097, 2 * 4096 + 1 and a masked 4-D one; mixed kinds, targets and scales."""
    xs = [R.make_case((n,), seed + i, device="cuda") for i, n in enumerate((1, 65, C + 1, 2 * C + 1))]
    x4, t4, w4 = R.make_case((2, 2, 8, 520), seed + 9, (2, 1, 8, 520), device="cuda")
    return [("mse", xs[0][0], xs[0][1], None, 1.0), ("l1", xs[1][0], 0.5, None, 2.0), ("l1", xs[2][0], xs[2][1], None, 0.05),
            ("mse", xs[3][0], 0, None, -0.3), ("mse", x4, t4, w4, 5.0)]


def _alone(term):
    from dvc_amd import losses
    return losses.fused([term])[1][0]


def test_fused_values_are_the_helpers_bits_in_any_order():
    from dvc_amd import losses
    terms = _five_terms()
    alone = torch.stack([_alone(tm) for tm in terms])
    for order in (list(range(5)), [4, 2, 0, 3, 1]):
        total, values = losses.fused([terms[i] for i in order])
        assert total.shape == () and values.shape == (5,) and values.dtype == total.dtype == torch.float32
        assert _bits_equal(values, alone[order]), order
        # the total: the float64 sum, in term order, of the S_k scale_k / n_k; formed here from the device's own fp32 values, so
        # the 5 roundings of those (2^-24 each, relative to sum |v_k|) and the total's own are the allowance — 1 ulp of the total
        # when no term cancels another (scales of mixed sign: measured against sum |v_k|)
        v64 = values.double().cpu()
        want = float(v64.sum())
        ulp = torch.finfo(torch.float32).eps * max(abs(want), float(v64.abs().sum()))
        assert abs(total.item() - want) <= ulp, (order, total.item(), want)
    # a helper is fused with a one-row table and scale 1: its result is the one-row total, with values[0]'s bits
    kind, x, t, w, _ = terms[4]
    tot1, val1 = losses.fused([(kind, x, t, w, 1.0)])
    assert _bits_equal(tot1, val1[0]) and _bits_equal(losses.weighted_mse_loss(x, t, w), tot1)
    for tm, a in zip(terms, alone):
        ref = R.term(*tm)
        assert R.value_error(a.item(), ref) <= R.C_VALUE, (tm[0], tm[1].shape)


def test_fused_backward_adds_the_upstream_gradients():
    from dvc_amd import losses
    terms = _five_terms(70)
    xs = [tm[1].clone().requires_grad_(True) for tm in terms]
    ts = [tm[2].clone().requires_grad_(True) if isinstance(tm[2], torch.Tensor) and i != 2 else tm[2] for i, tm in enumerate(terms)]
    total, values = losses.fused([(tm[0], x, t, tm[3], tm[4]) for tm, x, t in zip(terms, xs, ts)])
    (total + 2 * values[1]).backward()
    for k, (tm, x, t) in enumerate(zip(terms, xs, ts)):
        ref = R.term(tm[0], tm[1], tm[2], tm[3], tm[4], upstream=3.0 if k == 1 else 1.0)        # term 1: three times the coefficient
        assert R.grad_error(x.grad, ref) <= R.C_GRAD, k
        if isinstance(t, torch.Tensor) and t.requires_grad:
            assert _bits_equal(t.grad, -x.grad), k
    # through the values alone, and through one of them
    xs2 = [tm[1].clone().requires_grad_(True) for tm in terms]
    _, values = losses.fused([(tm[0], x, tm[2], tm[3], tm[4]) for tm, x in zip(terms, xs2)])
    values[3].backward()
    assert R.grad_error(xs2[3].grad, R.term(*terms[3])) <= R.C_GRAD
    assert all(bool((xs2[k].grad == 0).all()) for k in (0, 1, 2, 4))


def test_fused_is_reproducible_across_calls_and_staging_slots():
    from dvc_amd import losses
    terms = _five_terms(90)

    def run():
        xs = [tm[1].clone().requires_grad_(True) for tm in terms]
        total, values = losses.fused([(tm[0], x, tm[2], tm[3], tm[4]) for tm, x in zip(terms, xs)])
        (3 * total + values[2]).backward()
        return [total.detach().clone(), values.detach().clone()] + [x.grad for x in xs]

    first, second = run(), run()
    assert all(_bits_equal(a, b) for a, b in zip(first, second))
    # an unrelated call and allocation in between: the other staging buffer, other table sizes, other device addresses
    spare = torch.randn(12345, device="cuda")
    losses.l1_loss(spare)
    third = run()
    assert all(_bits_equal(a, b) for a, b in zip(first, third))


# ---- non-finite
def test_non_finite_inputs_stay_in_their_term():
    from dvc_amd import losses
    terms = _five_terms(110)
    clean = losses.fused(terms)[1].clone()
    for k, make in ((2, "nan"), (3, "inf-inf"), (4, "nan under a zero weight")):
        kind, x, t, w, scale = terms[k]
        x, t = x.clone(), t.clone() if isinstance(t, torch.Tensor) else t
        if make == "nan":
            x[C + 0] = float("nan")             # the last chunk of the 4097-element term: its only element
        elif make == "inf-inf":
            x[7] = float("inf")
            t = torch.zeros_like(x)
            t[7] = float("inf")
        else:
            w = w.clone()
            w[1, 0, 3, 17] = 0.0
            x[1, 1, 3, 17] = float("nan")
            torch_value = (((x - t) ** 2) * w.expand_as(x)).mean()
            assert torch.isnan(torch_value)     # torch's composition of the reference's expression does the same
        dirty = list(terms)
        dirty[k] = (kind, x, t, w, scale)
        total, values = losses.fused(dirty)
        assert torch.isnan(values[k]) and torch.isnan(total), make
        keep = [i for i in range(5) if i != k]
        assert _bits_equal(values[keep], clean[keep]), make


# ---- plumbing
@contextlib.contextmanager
def _count_calls():
    from dvc_amd import ops
    calls, real = [], (ops.loss_fwd, ops.loss_bwd)

    def fwd(*a, **kw):
        calls.append("fwd")
        return real[0](*a, **kw)

    def bwd(*a, **kw):
        calls.append("bwd")
        return real[1](*a, **kw)

    ops.loss_fwd, ops.loss_bwd = fwd, bwd
    try:
        yield calls
    finally:
        ops.loss_fwd, ops.loss_bwd = real


def test_one_forward_and_one_backward_call_whatever_the_terms():
    from dvc_amd import losses
    assert losses.CHUNK == C
    terms = _five_terms(130)
    for count in (1, 2, 5):
        xs = [tm[1].clone().requires_grad_(True) for tm in terms[:count]]
        with _count_calls() as calls:
            total, values = losses.fused([(tm[0], x, tm[2], tm[3], tm[4]) for tm, x in zip(terms, xs)])
            assert calls == ["fwd"]
            (total + values.sum()).backward()
            assert calls == ["fwd", "bwd"]
    with _count_calls() as calls:
        x = terms[1][1].clone().requires_grad_(True)
        losses.l1_loss(x).backward()
    assert calls == ["fwd", "bwd"]


def test_refused_inside_a_stream_capture_before_any_launch():
    from dvc_amd import losses
    x, t, _ = R.make_case((C + 1,), 150, device="cuda")
    want = losses.mse_loss(x, t).clone()
    torch.cuda.synchronize()
    graph, other = torch.cuda.CUDAGraph(), torch.zeros(8, device="cuda")
    with _count_calls() as calls:
        with torch.cuda.graph(graph):           # (capture runs on a side stream)
            other.add_(1.0)                     # an ordinary captured kernel: the capture itself is a normal one
            with pytest.raises(RuntimeError, match="cannot be captured into a graph"):
                losses.mse_loss(x, t)
            with pytest.raises(RuntimeError, match="cannot be captured into a graph"):
                losses.fused([("l1", x, t, None, 2.0)])
    torch.cuda.synchronize()
    assert calls == []
    assert _bits_equal(losses.mse_loss(x, t), want)


def test_on_a_side_stream():
    from dvc_amd import losses
    x, t, w = R.make_case((2, 2, 8, 520), 170, (2, 1, 8, 520), device="cuda")
    want = losses.weighted_mse_loss(x, t, w).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xs = x.clone().requires_grad_(True)
        loss = losses.weighted_mse_loss(xs, t, w)
        (3 * loss).backward()
        doubled = loss.detach() * 2             # consumed on the same stream
        grad = xs.grad.clone()
    side.synchronize()
    assert _bits_equal(loss.detach(), want) and doubled.item() == 2 * want.item()
    assert R.grad_error(grad, R.term("mse", x, t, w, upstream=3.0)) <= R.C_GRAD


def test_refusals_on_the_device():
    from dvc_amd import losses
    x = torch.randn(2, 3, 4, 5, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        losses.mse_loss(x.half())
    with pytest.raises(NotImplementedError, match="weights that require grad"):
        losses.weighted_mse_loss(x, x, torch.ones(2, 1, 4, 5, device="cuda", requires_grad=True))
    with pytest.raises(NotImplementedError, match="broadcasting weights of shape"):
        losses.weighted_l1_loss(x, x, torch.ones(2, 3, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="no elements"):
        losses.l1_loss(torch.zeros(0, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.mse_loss(x, torch.zeros(2, 3, 4, 5))


# ---- end to end
def test_colorvidnet_gradients_under_a_fused_two_term_loss():
    """ColorVidNet in training mode at the smallest input of tests/test_gpu_cvn_backward.py (2 x 48 x 80, contractive weights): an
    L1 term to a random target plus a masked MSE to a detached, shifted copy of the output, as one fused call — the 65 parameter
    gradients against the same network under the torch composition of the two terms, at that file's relative bound (1e-5)."""
    from dvc_amd import losses, synth
    from models.ColorVidNet import ColorVidNet
    B, H, W = 2, 48, 80
    with contextlib.redirect_stdout(io.StringIO()):
        m = ColorVidNet(7)
    m.load_state_dict(synth.colorvidnet_state_dict(0, contractive=True))
    m = m.cuda().train()
    g = torch.Generator().manual_seed(2)
    x = ((torch.rand(B, 7, H, W, generator=g) * 2 - 1) * 50).cuda()
    target = torch.randn(B, 2, H, W, generator=g).cuda()
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.7).float().cuda()

    def grads(fused):
        m.zero_grad(set_to_none=True)
        y = m(x)
        shifted = y.detach() + 0.1
        if fused:
            loss, _ = losses.fused([("l1", y, target, None, 1.0), ("mse", y, shifted, mask, 2.0)])
        else:
            loss = (y - target).abs().mean() + 2.0 * (((y - shifted) ** 2) * mask.expand_as(y)).mean()
        loss.backward()
        return loss.item(), {k: p.grad.clone() for k, p in m.named_parameters()}

    loss_f, got = grads(True)
    loss_t, want = grads(False)
    assert len(got) == 65 and abs(loss_f - loss_t) <= 1e-6 * abs(loss_t)
    worst = max((float((got[k].double() - want[k].double()).norm() / want[k].double().norm().clamp_min(1e-300)), k) for k in want)
    print("worst rel L2 over the 65 parameter gradients:", worst)
    assert worst[0] <= 1e-5, worst
