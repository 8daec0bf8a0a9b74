"""GPU: dvc_amd.losses.Plan / dvc_loss_plan_fwd, dvc_loss_plan_bwd (csrc/loss_plan.hip).  "l1" / "mse" terms bit for bit against
dvc_amd.losses.fused; "mean" and "rel" inside the bounds derived in tests/loss_plan_reference.py against float64, for values, dx,
dt and dy, and exactly on integer data; every term bit-identical alone and inside a six-term plan and from run to run; the resident
tables (a second call is launches only, a moved tensor is one upload); forward + backward + a GuardedAdam step replayed from one
graph against the eager sequence; non-finite inputs.  Sizes sit around the chunk (4096): 1, 5, 1023, 4095, 4096, 4097, 2 * 4096 + 3."""
import contextlib
import math
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_plan_reference as R  # noqa: E402
import losses_reference as L  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096
SIZES = [1, 5, 1023, 4095, 4096, 4097, 2 * C + 3]
NY = [1, 7, 4097]
MASKED = [((3, 2, 1, 5), (3, 1, 1, 5)),         # H * W % 4 != 0: the broadcast weight is read element by element
          ((2, 3, 2, 4), (2, 1, 2, 4)),         # H * W % 4 == 0: 16-byte loads of the broadcast weight
          ((2, 2, 8, 520), (2, 1, 8, 520))]     # plane 4160: the broadcast crosses chunk boundaries mid-image


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _misaligned(v):
    """The same values in a contiguous tensor whose storage starts one element (4 bytes) past a 16-byte boundary."""
    buf = torch.empty(v.numel() + 1, device=v.device)
    out = buf[1:].view(v.shape)
    out.copy_(v)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _leaf(v):
    """A leaf that shares v's storage (and so its alignment)."""
    return v.detach().requires_grad_(True)


def _randn(shape, seed, shift=0.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) + shift).cuda()


def _run(call, term, upstream=3.0):
    """One term through `call` (a Plan, or losses.fused): -> (value, grads of the tensors among term[1:3] in order)."""
    leaves = [_leaf(v) if isinstance(v, torch.Tensor) else v for v in term[1:3]]
    total, values = call([(term[0], leaves[0], leaves[1], term[3], term[4])])
    assert total.shape == () and values.shape == (1,) and _bits_equal(total, values[0]) and total.is_cuda
    (upstream * total).backward()
    return values[0].detach(), [v.grad for v in leaves if isinstance(v, torch.Tensor)]


# ---- "l1" / "mse": the bits of losses.fused
def _pixel_variants(n):
    """(label, x, t, w) over tensor and scalar targets, full weights, and each of x, t, w one element off 16-byte alignment."""
    x, t, w = _randn((n,), 10 + n), _randn((n,), 20 + n), _randn((n,), 30 + n)
    return [("aligned", x, t, None), ("scalar target", x, 0.5, None), ("weights", x, t, w), ("x off", _misaligned(x), t, w),
            ("t off", x, _misaligned(t), w), ("w off", x, t, _misaligned(w))]


@pytest.mark.parametrize("n", SIZES)
def test_l1_and_mse_have_the_bits_of_fused(n):
    from dvc_amd import losses
    plan = losses.Plan()
    for kind in ("l1", "mse"):
        for label, x, t, w in _pixel_variants(n):
            got_v, got_g = _run(plan, (kind, x, t, w, 0.75))
            want_v, want_g = _run(losses.fused, (kind, x, t, w, 0.75))
            assert torch.equal(got_v, want_v) and _bits_equal(got_v, want_v), (kind, n, label)
            assert len(got_g) == len(want_g) and all(torch.equal(a, b) and _bits_equal(a, b) for a, b in zip(got_g, want_g)), (kind, n, label)


@pytest.mark.parametrize("shape,mask", MASKED)
def test_masked_l1_and_mse_have_the_bits_of_fused(shape, mask):
    from dvc_amd import losses
    plan = losses.Plan()
    x, t, w = L.make_case(shape, 40 + sum(shape), mask, device="cuda")
    for kind in ("l1", "mse"):
        for xx, ww in ((x, w), (_misaligned(x), w), (x, _misaligned(w))):
            got_v, got_g = _run(plan, (kind, xx, t, ww, 2.0))
            want_v, want_g = _run(losses.fused, (kind, xx, t, ww, 2.0))
            assert torch.equal(got_v, want_v) and all(torch.equal(a, b) for a, b in zip(got_g, want_g)), (kind, shape)
            assert L.value_error(got_v.item(), L.term(kind, x, t, w, 2.0)) <= L.C_VALUE


# ---- "mean"
def _check_mean(plan, x, t, w, scale, label, expect=None):
    value, grads = _run(plan, ("mean", x, t, w, scale))
    ref = R.mean_term(x, t, w, scale, upstream=3.0)
    ev = abs(value.item() - ref["value64"]) / (R.EPS * ref["A"]) if ref["A"] > 0 else float(value.item() != ref["value64"])
    eg = R.mean_grad_error(grads[0], ref)
    print("mean", label, "value error / (EPS A) =", ev, " grad error / (EPS |dx64|) =", eg)
    assert ev <= R.C_MEAN_VALUE and eg <= R.C_MEAN_GRAD, (label, ev, eg)
    if isinstance(t, torch.Tensor):
        assert _bits_equal(grads[1], -grads[0]), label          # dt = -dx
    if expect is not None:
        assert _bits_equal(value, expect[0]) and _bits_equal(grads[0], expect[1]), label     # the path changes the loads, not the sum
    return value, grads[0]


@pytest.mark.parametrize("n", SIZES)
def test_mean_sizes_paths_and_targets(n):
    from dvc_amd import losses
    plan = losses.Plan()
    x, t, w = _randn((n,), 50 + n, 0.2), _randn((n,), 60 + n), _randn((n,), 70 + n)
    base = _check_mean(plan, x, t, None, -0.3, (n, "aligned"))
    _check_mean(plan, _misaligned(x), t, None, -0.3, (n, "x off"), base)
    _check_mean(plan, x, _misaligned(t), None, -0.3, (n, "t off"), base)
    based = _check_mean(plan, x, t, w, -0.3, (n, "signed weights"))
    _check_mean(plan, x, t, _misaligned(w), -0.3, (n, "w off"), based)
    v0, g0 = _check_mean(plan, x, 0, None, 0.1, (n, "target 0"))         # INTEGRATION.md's use: w_ctx * mean(per-sample losses)
    want = 0.1 * x.double().mean().item()
    assert abs(v0.item() - want) <= 4 * R.EPS * 0.1 * x.double().abs().mean().item()
    assert bool((g0.view(torch.int32) == g0.view(torch.int32)[0]).all())        # one coefficient for every element


@pytest.mark.parametrize("shape,mask", MASKED)
def test_mean_with_a_broadcast_mask(shape, mask):
    from dvc_amd import losses
    plan = losses.Plan()
    for signed in (False, True):
        x, t, w = L.make_case(shape, 80 + sum(shape), mask, signed, device="cuda")
        base = _check_mean(plan, x, t, w, 1.5, (shape, signed))
        _check_mean(plan, _misaligned(x), t, _misaligned(w), 1.5, (shape, signed, "off"), base)
        if not signed:
            assert bool((base[1][w.expand_as(x) == 0] == 0).all())


# ---- "rel"
def _check_rel(plan, x, y, c, scale, label, expect=None):
    xl, yl = _leaf(x), _leaf(y)
    total, values = plan([("rel", xl, yl, c, scale)])
    (3 * total).backward()
    ref = R.rel_term(x, y, c, scale, upstream=3.0)
    ev, ex, ey = R.rel_errors(values[0].item(), xl.grad, yl.grad, ref)
    print("rel", label, "fractions of the bounds: value", ev, "dx", ex, "dy", ey)
    assert ev <= 1.0 and ex <= 1.0 and ey <= 1.0, (label, ev, ex, ey)
    assert xl.grad.shape == x.shape and yl.grad.shape == y.shape
    assert bool((yl.grad.view(torch.int32) == yl.grad.view(torch.int32).reshape(-1)[0]).all())      # dy is one value
    if expect is not None:
        assert all(_bits_equal(a, b) for a, b in zip((values[0].detach(), xl.grad, yl.grad), expect)), label
    return values[0].detach(), xl.grad, yl.grad


@pytest.mark.parametrize("n_y", NY)
@pytest.mark.parametrize("n", SIZES)
def test_rel_against_float64_and_against_torch(n, n_y):
    from dvc_amd import losses
    plan = losses.Plan()
    x, y = _randn((n,), 90 + n, 0.4), _randn((n_y,), 100 + n_y, -0.2)
    for c, scale in ((-1.0, 0.5), (1.0, 0.5)):
        base = _check_rel(plan, x, y, c, scale, (n, n_y, c))
        lit = R.torch_rel(x, y, c, R._f32(scale)).item()        # INTEGRATION.md's expression, literally
        assert abs(base[0].item() - lit) <= R.rel_term(x, y, c, scale)["value_bound"] + R.torch_rel_bound(x, y, c, scale), (n, n_y, c)
    _check_rel(plan, _misaligned(x), y, 1.0, 0.5, (n, n_y, "x off"), base)
    _check_rel(plan, x, _misaligned(y), 1.0, 0.5, (n, n_y, "y off"), base)
    if n == SIZES[-1]:      # shapes are free: a [B, 1] discriminator output against a 4-D one of another size
        v = _check_rel(plan, x.view(n, 1), y.view(1, n_y, 1, 1), 1.0, 0.5, (n, n_y, "shapes"), None)
        assert _bits_equal(v[0], base[0]) and _bits_equal(v[1].view(-1), base[1]) and _bits_equal(v[2].view(-1), base[2])
        from dvc_amd.losses import relativistic_loss
        xl = _leaf(x)
        one = relativistic_loss(xl, y, 1.0)
        (1.5 * one).backward()
        assert _bits_equal((one.detach().double() * 0.5).float(), base[0]) and _bits_equal(xl.grad, base[1])    # scale 1 vs 0.5: exact


def test_only_the_side_that_requires_grad_gets_one():
    from dvc_amd import losses
    plan = losses.Plan()
    x, y = _randn((C + 1,), 1), _randn((7,), 2)
    both = _check_rel(plan, x, y, -1.0, 0.5, "both")
    yl = _leaf(y)
    total, _ = plan([("rel", x, yl, -1.0, 0.5)])
    (3 * total).backward()
    assert x.grad is None and _bits_equal(yl.grad, both[2])
    xl = _leaf(x)
    total, _ = plan([("rel", xl, y, -1.0, 0.5)])
    (3 * total).backward()
    assert y.grad is None and _bits_equal(xl.grad, both[1])
    assert not plan([("rel", x, y, -1.0, 0.5)])[0].requires_grad


# ---- exact cases
@pytest.mark.parametrize("n,n_y", [(1, 1), (5, 8), (C + 1, 4096), (2 * C + 3, 64), (1024, 4096)])
def test_integer_data_is_exact(n, n_y):
    """Integers in +-2^10 with mean(y) an integer (n_y a power of two, one element adjusted): every fp32 operation of the kernel is
    exact, so value, dx and dy are the int64 results pushed through the same double expressions and rounded once."""
    from dvc_amd import losses
    g = torch.Generator().manual_seed(7 * n + n_y)
    xi = torch.randint(-1024, 1025, (n,), generator=g)
    yi = torch.randint(-1024, 1025, (n_y,), generator=g)
    yi[0] -= int(yi.sum()) % n_y
    assert int(yi.sum()) % n_y == 0 and int(yi.abs().max()) < 1024 + n_y        # |d| < 2^12: d * d is exact in fp32
    m, c, scale = int(yi.sum()) // n_y, -1, 0.5
    d = xi - m - c
    S, Sd = int((d * d).sum()), int(d.sum())
    xl, yl = _leaf(xi.float().cuda()), _leaf(yi.float().cuda())
    plan = losses.Plan()
    total, values = plan([("rel", xl, yl, float(c), scale)])
    total.backward()
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()        # one rounding
    assert values[0].item() == f32(S * scale / n).item()
    coef = f32(1.0 * scale / n).item()
    assert torch.equal(xl.grad.cpu(), (2.0 * coef * d.double()).float())
    assert torch.equal(yl.grad.cpu(), torch.full((n_y,), f32(-(2.0 * coef) * Sd / n_y).item()))
    # "mean": w * (x - t) on integers, w in {-3 .. 3}
    ti, wi = torch.randint(-1024, 1025, (n,), generator=g), torch.randint(-3, 4, (n,), generator=g)
    xm = _leaf(xi.float().cuda())
    total, values = plan([("mean", xm, ti.float().cuda(), wi.float().cuda(), 0.25)])
    total.backward()
    assert values[0].item() == f32(int((wi * (xi - ti)).sum()) * 0.25 / n).item()
    assert torch.equal(xm.grad.cpu(), (f32(0.25 / n).item() * wi.double()).float())


def test_a_sum_of_d_that_needs_more_than_24_bits_reaches_dy_exactly():
    """One element 2^30 among 8191 ones, mean(y) = 0, c = 0: every d and every product with a power-of-two coefficient is exact in
    fp32, but sum d = 2^30 + 8191 has 31 significant bits — it survives only because it is accumulated and kept in double; dy is
    that integer pushed through the kernel's double expression and rounded once."""
    from dvc_amd import losses
    n, n_y, scale = 2 * C, 1, 0.5
    xi = torch.ones(n, dtype=torch.int64)
    xi[0] = 2 ** 30
    xl, yl = _leaf(xi.float().cuda()), _leaf(torch.zeros(n_y, device="cuda"))
    total, _ = losses.Plan()([("rel", xl, yl, 0.0, scale)])
    total.backward()
    coef = scale / n                                    # a power of two
    want_dy = torch.tensor(-(2.0 * coef) * int(xi.sum()) / n_y, dtype=torch.float64).float()
    assert want_dy.double().item() == -(2.0 * coef) * (2 ** 30 + 8192)      # (the one rounding: 8191 -> 8192 at this magnitude)
    assert torch.equal(yl.grad.cpu(), want_dy.reshape(1))
    assert torch.equal(xl.grad.cpu(), (2.0 * coef * xi.double()).float())
    s2 = 2 ** 60 + (n - 1)                              # sum d^2: past a double's 53 bits, so the value is held to its bound only
    assert abs(total.item() - s2 * scale / n) <= R.rel_term(xl.detach(), yl.detach(), 0.0, scale)["value_bound"]


# ---- alone, inside a six-term plan, twice
def _six(seed):
    x4, t4, w4 = L.make_case((2, 2, 8, 520), seed, (2, 1, 8, 520), device="cuda")
    fake_x, real_y = _randn((7, 1), seed + 1, 0.3), _randn((C + 1,), seed + 2, -0.1)
    real_x, fake_y = _randn((C + 1,), seed + 3, -0.1), _randn((7, 1), seed + 4, 0.3)
    return [("l1", _randn((C + 1,), seed + 5), _randn((C + 1,), seed + 6), None, 1.0),
            ("mse", _randn((2 * C + 3,), seed + 7), 0.5, None, 0.2),
            ("mse", x4, t4, w4, 2.0),
            ("mean", _randn((5,), seed + 8, 1.0), 0, None, 0.1),
            ("rel", fake_x, real_y, -1.0, 0.25),
            ("rel", real_x, fake_y, 1.0, 0.25)]


def _run_all(plan, terms, weights):
    leaves = [[_leaf(v) if isinstance(v, torch.Tensor) else v for v in tm[1:3]] for tm in terms]
    total, values = plan([(tm[0], lv[0], lv[1], tm[3], tm[4]) for tm, lv in zip(terms, leaves)])
    (total + sum(wk * values[k] for k, wk in enumerate(weights))).backward()
    return total.detach().clone(), values.detach().clone(), [[v.grad for v in lv if isinstance(v, torch.Tensor)] for lv in leaves]


def test_every_term_is_bit_identical_alone_inside_six_and_twice():
    from dvc_amd import losses
    terms, weights = _six(200), [0.0, 2.0, 0.0, 1.0, 0.5, 0.0]
    plan = losses.Plan()
    total, values, grads = _run_all(plan, terms, weights)
    total2, values2, grads2 = _run_all(plan, terms, weights)
    assert _bits_equal(total, total2) and _bits_equal(values, values2)
    assert all(_bits_equal(a, b) for ga, gb in zip(grads, grads2) for a, b in zip(ga, gb))
    order = [5, 3, 1, 4, 0, 2]
    _, values_r, grads_r = _run_all(losses.Plan(), [terms[i] for i in order], [weights[i] for i in order])
    assert _bits_equal(values_r, values[order])
    assert all(_bits_equal(a, b) for j, i in enumerate(order) for a, b in zip(grads_r[j], grads[i]))
    for k, tm in enumerate(terms):
        v, g = _run(losses.Plan(), tm, upstream=1.0 + weights[k])
        assert _bits_equal(v, values[k]), k
        assert len(g) == len(grads[k]) and all(_bits_equal(a, b) for a, b in zip(g, grads[k])), k
    v64 = values.double().cpu()
    assert abs(total.item() - float(v64.sum())) <= torch.finfo(torch.float32).eps * float(v64.abs().sum())
    # the two unchanged kinds also against fused, inside the plan
    fused_values = losses.fused(terms[:3])[1]
    assert _bits_equal(fused_values, values[:3])
    for k in (4, 5):
        ref = R.rel_term(terms[k][1], terms[k][2], terms[k][3], terms[k][4], upstream=1.0 + weights[k])
        assert max(R.rel_errors(values[k].item(), grads[k][0], grads[k][1], ref)) <= 1.0, k


# ---- residency
@contextlib.contextmanager
def _recorded():
    """The library calls a Plan makes and every host-to-device Tensor.copy_, in order."""
    from dvc_amd import ops
    log, real = [], (ops.loss_plan_fwd, ops.loss_plan_bwd, ops.loss_plan_check, torch.Tensor.copy_)

    def wrap(name, fn):
        def logged(*a, **kw):
            log.append(name)
            return fn(*a, **kw)
        return logged

    def copy_(self, src, *a, **kw):
        if self.is_cuda and isinstance(src, torch.Tensor) and not src.is_cuda:
            log.append("h2d")
        return real[3](self, src, *a, **kw)

    ops.loss_plan_fwd, ops.loss_plan_bwd, ops.loss_plan_check = wrap("fwd", real[0]), wrap("bwd", real[1]), wrap("check", real[2])
    torch.Tensor.copy_ = copy_
    try:
        yield log
    finally:
        ops.loss_plan_fwd, ops.loss_plan_bwd, ops.loss_plan_check, torch.Tensor.copy_ = real


def test_an_unchanged_call_is_launches_only_and_a_moved_tensor_is_one_upload():
    from dvc_amd import losses
    terms = _six(300)
    leaves = [[_leaf(v) if isinstance(v, torch.Tensor) else v for v in tm[1:3]] for tm in terms]
    live = [(tm[0], lv[0], lv[1], tm[3], tm[4]) for tm, lv in zip(terms, leaves)]
    plan = losses.Plan()

    def step(tms):
        for tm in tms:
            for v in tm[1:3]:
                if isinstance(v, torch.Tensor):
                    v.grad = None           # (the allocator hands the next backward the same addresses)
        with _recorded() as log:
            total, values = plan(tms)
            total.backward()
        where = tuple(v.grad.data_ptr() for tm in tms for v in tm[1:3] if isinstance(v, torch.Tensor))
        return values.detach().clone(), where, log

    first, where, log = step(live)
    assert log == ["check", "h2d", "fwd", "check", "h2d", "bwd"] and plan.uploads == 2
    stayed = 0
    for _ in range(4):
        # The inputs did not move: the forward is its launches, no check, no copy, no rebuild.  The backward's tables also name the
        # gradients, which the allocator places: where it hands out the addresses of the step before (what a steady loop settles
        # into) the backward is its launch only, and where it does not, exactly one rebuild and one upload.
        again, now, log = step(live)
        assert log == ["fwd"] + (["bwd"] if now == where else ["check", "h2d", "bwd"]), (log, now == where)
        assert _bits_equal(again, first)
        stayed += now == where
        where = now
    print("backward fingerprint hits in 4 repeated steps:", stayed)
    uploads = plan.uploads
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    with _recorded() as log, torch.no_grad():
        plan(live)
    assert log == ["fwd"] and plan.uploads == uploads
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated + 1        # the outputs, nothing else
    # one input replaced by a new tensor: exactly one upload, of the forward's tables
    moved = list(live)
    moved[1] = ("mse", live[1][1].detach().clone(), 0.5, None, 0.2)
    assert moved[1][1].data_ptr() != live[1][1].data_ptr()
    with _recorded() as log, torch.no_grad():
        changed = plan(moved)[1]
    assert log == ["check", "h2d", "fwd"] and plan.uploads == uploads + 1 and _bits_equal(changed, first)
    with _recorded() as log, torch.no_grad():
        plan(moved)
    assert log == ["fwd"]
    # a changed scalar is a rebuild too, and the value follows it
    moved[4] = ("rel", moved[4][1], moved[4][2], 1.0, 0.25)
    with _recorded() as log, torch.no_grad():
        flipped = plan(moved)[1]
    assert log == ["check", "h2d", "fwd"] and not _bits_equal(flipped[4], first[4]) and _bits_equal(flipped[:4], first[:4])


def test_a_backward_after_the_plan_ran_again_is_refused_for_relativistic_terms():
    from dvc_amd import losses
    plan = losses.Plan()
    x, y = _leaf(_randn((5,), 1)), _randn((7,), 2)
    first = plan([("rel", x, y, 1.0, 1.0)])[0]
    plan([("rel", x, y, 1.0, 1.0)])
    with pytest.raises(RuntimeError, match="one Plan per call site"):
        first.backward()
    a = plan([("mse", x, 0, None, 1.0)])[0]         # no relativistic term: nothing is kept in the scratch
    plan([("mse", x, 0, None, 1.0)])
    a.backward()


# ---- capture
def _step_data(it):
    return dict(t1=_randn((2, 2, 8, 520), 400 + it), t2=_randn((2, 2, 8, 520), 500 + it),
                mask=(torch.rand(2, 1, 8, 520, generator=torch.Generator().manual_seed(600 + it)) < 0.6).float().cuda(),
                real=_randn((C + 1,), 700 + it, 0.5))


def _train_terms(params, d):
    ab, cx, fake = params
    return [("l1", ab, d["t1"], None, 1.0), ("mse", ab, d["t2"], d["mask"], 2.0), ("mean", cx, 0, None, 0.1),
            ("rel", fake, d["real"], -1.0, 0.25), ("rel", d["real"], fake, 1.0, 0.25)]


def _new_params():
    return [torch.nn.Parameter(_randn(s, 800 + i)) for i, s in enumerate(((2, 2, 8, 520), (5,), (7, 1)))]


def test_forward_backward_and_guarded_step_replay_from_one_graph():
    """One eager iteration, then loss + backward + GuardedAdam.step() captured into ONE graph; new data written into the same
    tensors before each of three replays; values, gradients and parameters against the same four iterations run eagerly."""
    from dvc_amd import losses, optim
    kw = dict(lr=1e-2, betas=(0.5, 0.999), max_grad_norm=1.0)
    data = [_step_data(it) for it in range(4)]
    # the eager sequence
    twins = _new_params()
    ref_opt, ref_plan, want = optim.GuardedAdam(twins, **kw), losses.Plan(), []
    for d in data:
        ref_opt.zero_grad(set_to_none=True)
        total, values = ref_plan(_train_terms(twins, d))
        total.backward()
        ref_opt.step()
        want.append((total.detach().clone(), values.detach().clone(), [p.grad.clone() for p in twins], [p.detach().clone() for p in twins]))
    # the captured one
    params = _new_params()
    opt, plan = optim.GuardedAdam(params, **kw), losses.Plan()
    static = {k: v.clone() for k, v in data[0].items()}
    total, values = plan(_train_terms(params, static))     # the eager call: tables, spares, optimiser state
    total.backward()
    opt.step()
    assert _bits_equal(values.detach(), want[0][1]) and all(_bits_equal(p.detach(), q) for p, q in zip(params, want[0][3]))
    opt.zero_grad(set_to_none=True)
    # The eager iteration's outputs go before the capture: while they live, their autograd graph keeps the parameters' gradient
    # accumulators, which belong to the stream that iteration ran on — the captured backward would hop to that stream and back
    # through events, and the captured region would no longer be a straight line on the capture's stream.
    del total, values
    torch.cuda.synchronize()
    uploads = plan.uploads
    graph = torch.cuda.CUDAGraph()
    with _recorded() as log, warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.cuda.graph(graph):
            total, values = plan(_train_terms(params, static))
            total.backward()
            opt.step()
    # torch warns when a backward node has to hop to another stream (an accumulator left over from the eager iteration): none did
    assert not [w for w in caught if "stream" in str(w.message).lower()], [str(w.message) for w in caught]
    # the forward's tables did not move; the backward's name gradients that live in the graph's pool: one captured upload
    assert [e for e in log if e != "h2d"] == ["fwd", "check", "bwd"] and plan.uploads == uploads + 1
    assert all(r.captured for r in plan._resident) and plan._resident[1].pinned is not None and len(plan._captured) == 2
    torch.cuda.synchronize()
    assert all(_bits_equal(p.detach(), q) for p, q in zip(params, want[0][3]))      # a capture runs nothing
    for it in (1, 2, 3):
        for k, v in data[it].items():
            static[k].copy_(v)
        graph.replay()
        opt.mark_updated()
        torch.cuda.synchronize()
        w_total, w_values, w_grads, w_params = want[it]
        assert torch.equal(total.detach(), w_total) and torch.equal(values.detach(), w_values), it
        assert all(torch.equal(p.grad, g) for p, g in zip(params, w_grads)), it
        assert all(torch.equal(p.detach(), q) for p, q in zip(params, w_params)), it
    assert opt.skipped_steps.item() == 0 and ref_opt.skipped_steps.item() == 0
    # and the plan goes on eagerly afterwards, with its spares replaced
    with torch.no_grad():
        assert _bits_equal(plan(_train_terms(twins, data[3]))[1], ref_plan(_train_terms(twins, data[3]))[1])
    assert len(plan._spares) == 2 and len(plan._captured) == 2


def test_a_capture_without_a_spare_says_to_call_the_plan_eagerly_once():
    from dvc_amd import losses
    x, y = _randn((5,), 1), _randn((7,), 2)
    plan, hinted = losses.Plan(), losses.Plan(n_terms_hint=2)
    assert plan._spares == [] and len(hinted._spares) == 2
    torch.cuda.synchronize()
    graph, out = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="call the plan eagerly once"):
            plan([("rel", x, y, 1.0, 1.0)])
        out.append(hinted([("rel", x, y, 1.0, 1.0), ("mean", x, 0, None, 1.0)])[1])         # the hint's spare serves the upload
    want = losses.Plan()([("rel", x, y, 1.0, 1.0), ("mean", x, 0, None, 1.0)])[1].clone()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(out[0], want)
        x.mul_(2.0)
        want = losses.Plan()([("rel", x, y, 1.0, 1.0), ("mean", x, 0, None, 1.0)])[1].clone()
    assert plan.uploads == 0 and hinted.uploads == 1


# ---- non-finite
def test_nan_under_a_zero_mask_stays_and_a_nan_in_y_skips_the_guarded_step():
    from dvc_amd import losses, optim
    d = _step_data(9)
    params = _new_params()
    plan = losses.Plan()
    clean = plan(_train_terms(params, d))[1].detach().clone()
    assert bool(torch.isfinite(clean).all())
    # a NaN where the mask is 0: the masked terms are NaN, as torch's composition is, and nothing else moves
    d["mask"][1, 0, 3, 17] = 0.0
    with torch.no_grad():
        params[0][1, 1, 3, 17] = math.nan
    assert torch.isnan((((params[0] - d["t2"]) ** 2) * d["mask"].expand_as(params[0])).mean())
    values = plan(_train_terms(params, d))[1].detach()
    masked_mean = plan([("mean", params[0].detach(), d["t2"], d["mask"], 1.0)])[1]
    assert torch.isnan(values[0]) and torch.isnan(values[1]) and torch.isnan(masked_mean[0]) and _bits_equal(values[2:], clean[2:])
    # a NaN in y: the relativistic value is NaN, its gradients are, and the guarded step skips itself
    params = _new_params()
    opt, plan = optim.GuardedAdam(params, lr=1e-2), losses.Plan()
    d = _step_data(10)
    d["real"][C] = math.nan             # the last chunk of y: its only element
    before = [p.detach().clone() for p in params]
    total, values = plan(_train_terms(params, d))
    total.backward()
    opt.step()
    assert torch.isnan(values[3]) and torch.isnan(values[4]) and torch.isnan(total) and bool(torch.isfinite(values[:3]).all())
    assert bool(torch.isnan(params[2].grad).all()) and bool(torch.isfinite(params[0].grad).all())
    assert opt.skipped_steps.item() == 1 and all(_bits_equal(p.detach(), q) for p, q in zip(params, before))
