"""Restatement of Discriminator_x64's parameter gradients (dvc_amd/gan.py behind set_parameter_training, csrc/gan_wgrad.hip) in
plain torch on the CPU, in the dtype it is given, with hand-written formulas — no autograd — on top of tests/gan_reference.py,
whose forward cache it reuses: the weight gradient of the 4x4 stride-2 layer, the spectral-norm backward

    d loss / d W_bar = G / sigma - (<G, W_bar> / sigma^2) u' v'^T        (u', v': the vectors AFTER the forward's power step)

`last`, the three 1x1 projections and gamma.  `param_grads` returns a dict keyed by state_dict name.

Next to it an INDEPENDENT autograd composition that spells the reference's SpectralNorm literally (`autograd_forward`): the power
step on u / v outside the graph, sigma = u' . (W_bar v') inside it, F.conv2d(x, W_bar / sigma, b, 2, 1), torch.softmax, the mean
of `last`.  tests/test_gan_train_host.py checks one against the other in float64; tools/gan_probe.py times the composition on
the device in float32.

`defect` seeds a known mistake: "no_sigma_grad" drops the rank-one term, "stale_uv" builds it from the u, v of BEFORE the power
step, "tap" exchanges ky and kx in the weight gradient, "gamma_x" takes d gamma with x instead of o."""
import torch
import torch.nn.functional as F

import gan_reference as R

SN_PREFIXES = tuple(f"{n}.0.module" for n in R.LAYERS) + tuple(f"attention.{n}.module" for n in R.ATT) + ("last.module",)
PARAM_NAMES = tuple(f"{p}.{k}" for p in SN_PREFIXES[:6] for k in ("weight_bar", "bias")) + \
    tuple(f"{p}.{k}" for p in SN_PREFIXES[6:9] for k in ("weight_bar", "bias")) + ("attention.gamma",) + \
    ("last.module.weight_bar", "last.module.bias")


def conv4s2_wgrad(dz, x, defect=None):
    """(G [Cout, Cin, 4, 4], db [Cout]): G[co][ci][ky][kx] = sum dz[n][co][oy][ox] x[n][ci][2 oy + ky - 1][2 ox + kx - 1]."""
    (N, Cout, OH, OW), Cin = dz.shape, x.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    G = dz.new_zeros((Cout, Cin, 4, 4))
    for ky in range(4):
        for kx in range(4):
            patch = xp[:, :, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]
            g = torch.einsum("nohw,nchw->oc", dz, patch)
            if defect == "tap":
                G[:, :, kx, ky] = g
            else:
                G[:, :, ky, kx] = g
    return G, dz.sum((0, 2, 3))


def sn_wgrad(G, w_bar, u, v, sigma, defect=None):
    """d loss / d W_bar from the plain weight gradient G; u, v after the power step."""
    if defect == "no_sigma_grad":
        return G / sigma
    W = w_bar.reshape(w_bar.shape[0], -1)
    c = (G.reshape(W.shape) * W).sum() / sigma
    return ((G.reshape(W.shape) - c * torch.outer(u, v)) / sigma).view_as(w_bar)


def last_wgrad(g, x):
    """(G [1, C, 3, 6], db [1]) of R.last_fwd for g [N, 1]."""
    N, C, H, W = x.shape
    OH, OW = H - 2, W - 5
    G = x.new_zeros((1, C, 3, 6))
    for ky in range(3):
        for kx in range(6):
            G[0, :, ky, kx] = (x[:, :, ky:ky + OH, kx:kx + OW].sum((2, 3)) * g.view(N, 1)).sum(0) / (OH * OW)
    return G, g.sum().view(1)


def attention_out(c):
    """(o [N, C, P], y [N, C, h, w]) of the attention block from the forward cache."""
    q, k, v, a = c["att"]
    o = v @ a.transpose(1, 2)
    return o, c["gamma"] * o.view(c["act"][4].shape) + c["act"][4]


def param_grads(sd, c, x, g_out=None, g_f4=None, defect=None):
    """(dx, {state_dict name: gradient}, scale) from the cache c of R.forward(sd, x) for the gradients at the two outputs.  A
    parameter no seeded output depends on gets a zero tensor.
    scale: the magnitude an error is to be measured against for the two gradients that are sums with cancellation, where the
    size of the result says nothing about the size of the rounding error: d gamma = sum dy o is measured against sum |dy o|;
    d bias of key_conv is ZERO in exact arithmetic (a bias on k adds q_i . b to every energy of row i, which the softmax over
    that row does not see: sum_j dE[i][j] = 0), so what is computed is rounding noise, measured against max_c sum |dk[c]|."""
    act, sig, w = c["act"], c["sigma"], c["w"]
    dt = act[1].dtype
    x = x.to(dt)
    grads, scale = {}, {}

    def sn(prefix, G, db, w_bar, sigma):
        u, v = c["uv"][prefix]
        if defect == "stale_uv":
            u, v = sd[prefix + ".weight_u"].to(dt), sd[prefix + ".weight_v"].to(dt)
        grads[prefix + ".weight_bar"], grads[prefix + ".bias"] = sn_wgrad(G, w_bar, u, v, sigma, defect), db

    d4 = None
    if g_out is not None:
        g = g_out.to(dt)
        sn("last.module", *last_wgrad(g, act[6]), c["w_last"], c["s_last"])
        d = R.last_bwd(g, c["w_last"], c["s_last"], act[6].shape) * R.lrelu_grad(act[6])
        sn("layer6.0.module", *conv4s2_wgrad(d, act[5], defect), w[6], sig[6])
        d = R.conv4s2_dgrad(d, w[6], sig[6], act[5].shape[2:]) * R.lrelu_grad(act[5])
        o, y = attention_out(c)
        sn("layer5.0.module", *conv4s2_wgrad(d, y, defect), w[5], sig[5])
        dy = R.conv4s2_dgrad(d, w[5], sig[5], act[4].shape[2:])
        # the attention block: gamma, then the three projections from [dq, dk, dv] against the block's input
        N, C, h, wd = dy.shape
        dyf, xf = dy.reshape(N, C, h * wd), act[4].reshape(N, C, h * wd)
        grads["attention.gamma"] = (dyf * (xf if defect == "gamma_x" else o)).sum().view(1)
        scale["attention.gamma"] = (dyf * o).abs().sum().item()
        q, k, v, a = c["att"]
        for name, W, s, dp in zip(R.ATT, c["att_w"], c["att_s"], R.attention_core_bwd(q, k, v, a, c["gamma"] * dyf)):
            G = torch.einsum("nop,ncp->oc", dp, xf).view(C, C, 1, 1)
            sn(f"attention.{name}.module", G, dp.sum((0, 2)), W, s)
            if name == "key_conv":
                scale["attention.key_conv.module.bias"] = dp.abs().sum((0, 2)).max().item()
        d4 = R.attention_bwd(c["att"], c["att_w"], c["att_s"], c["gamma"], dy)
    if g_f4 is not None:
        d4 = g_f4.to(dt) if d4 is None else d4 + g_f4.to(dt)
    d = d4 * R.lrelu_grad(act[4])
    for i in (4, 3, 2):
        sn(f"layer{i}.0.module", *conv4s2_wgrad(d, act[i - 1], defect), w[i], sig[i])
        d = R.conv4s2_dgrad(d, w[i], sig[i], act[i - 1].shape[2:]) * R.lrelu_grad(act[i - 1])
    sn("layer1.0.module", *conv4s2_wgrad(d, x, defect), w[1], sig[1])
    for n in PARAM_NAMES:
        if n not in grads:
            grads[n] = torch.zeros_like(sd[n], dtype=dt)
    return R.conv4s2_dgrad(d, w[1], sig[1], c["x_shape"][2:]), grads, scale


def advance(sd, c):
    """The state_dict after the forward that made cache c: weight_u / weight_v replaced by the updated vectors."""
    sd2 = dict(sd)
    for prefix, (u, v) in c["uv"].items():
        sd2[prefix + ".weight_u"], sd2[prefix + ".weight_v"] = u, v
    return sd2


def relativistic_ls_seeds(r, f):
    """(d L / d r, d L / d f) of train.py's discriminator loss L = (mean((r - mean f - 1)^2) + mean((f - mean r + 1)^2)) / 2."""
    A, B = r - f.mean() - 1, f - r.mean() + 1
    return (A - B.mean()) / r.numel(), (B - A.mean()) / f.numel()


def relativistic_ls_loss(r, f):
    return (torch.mean((r - torch.mean(f) - 1) ** 2) + torch.mean((f - torch.mean(r) + 1) ** 2)) / 2


# ------------------------------------------------------------------------------------------------ the autograd composition
def leaf_params(sd, dtype=torch.float64, device="cpu"):
    """({name: leaf tensor requiring grad} for the 21 parameters, {prefix: [u, v]} the power-iteration state)."""
    params = {n: sd[n].to(device=device, dtype=dtype).clone().requires_grad_(True) for n in PARAM_NAMES}
    uv = {p: [sd[p + ".weight_u"].to(device=device, dtype=dtype).clone(), sd[p + ".weight_v"].to(device=device, dtype=dtype).clone()]
          for p in SN_PREFIXES}
    return params, uv


def _spectral_weight(params, uv, prefix):
    """SpectralNorm._update_u_v, literally: one power step on u.data / v.data, then sigma = u . (W v) in the graph."""
    w = params[prefix + ".weight_bar"]
    height = w.shape[0]
    u, v = uv[prefix]
    with torch.no_grad():
        wm = w.view(height, -1)
        v = R.l2n(torch.mv(wm.t(), u))
        u = R.l2n(torch.mv(wm, v))
        uv[prefix] = [u, v]
    sigma = u.dot(w.view(height, -1).mv(v))
    return w / sigma.expand_as(w)


def autograd_forward(params, uv, x):
    """(output, feature4) under autograd; uv is advanced in place, as every forward of the reference does."""
    a = x
    for name in R.LAYERS:
        p = name + ".0.module"
        a = F.leaky_relu(F.conv2d(a, _spectral_weight(params, uv, p), params[p + ".bias"], 2, 1), R.SLOPE)
        if name == "layer4":
            f4 = a
            N, C, h, w = a.shape
            q, k, v = (F.conv2d(a, _spectral_weight(params, uv, f"attention.{n}.module"),
                                params[f"attention.{n}.module.bias"]).view(N, C, h * w) for n in R.ATT)
            att = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=-1)
            a = params["attention.gamma"] * torch.bmm(v, att.transpose(1, 2)).view(N, C, h, w) + a
    out = F.conv2d(a, _spectral_weight(params, uv, "last.module"), params["last.module.bias"]).mean((2, 3)).view(-1, 1)
    return out, f4


def autograd_grads(sd, x, g_out=None, g_f4=None, forwards=1):
    """(dx, {name: gradient}) in float64 from the composition; forwards = 2 runs one forward first (its graph is dropped) and
    differentiates the second."""
    params, uv = leaf_params(sd)
    x = x.double().clone().requires_grad_(True)
    for _ in range(forwards):
        out, f4 = autograd_forward(params, uv, x)
    loss = 0
    if g_out is not None:
        loss = loss + (out * g_out.double()).sum()
    if g_f4 is not None:
        loss = loss + (f4 * g_f4.double()).sum()
    loss.backward()
    return x.grad, {n: torch.zeros_like(p) if p.grad is None else p.grad for n, p in params.items()}
