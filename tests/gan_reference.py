"""Restatement of Discriminator_x64 (dvc_amd/gan.py, csrc/gan.hip) in plain torch on the CPU, in the dtype it is given (float64:
the reference of the GPU tests; float32: their yardstick), with hand-written backward formulas — no autograd.  Piece by piece:
the spectral-norm power step, the 4x4 stride-2 layer and its input gradient in gather form (2 x 2 taps per output channel, chosen
by the parity of the input pixel), the attention block and its backward, `last` and its backward, and the whole network.
tests/test_gan_host.py checks all of it against float64 autograd through a composition of nn.Conv2d and softmax.

`defect` seeds a known mistake (the host test shows that the comparison catches each): "parity" takes the taps of the wrong
row parity in the input gradient, "sigma_bias" divides the bias by sigma too, "softmax_sum" drops the sum_j term of the softmax
backward, "mean" divides `last` by the filter size instead of the number of positions."""
import torch
import torch.nn.functional as F

SLOPE = 0.2
EPS = 1e-12
LAYERS = ("layer1", "layer2", "layer3", "layer4", "layer5", "layer6")
ATT = ("query_conv", "key_conv", "value_conv")


def l2n(z):
    return z / (z.norm() + EPS)


def sigma_step(w_bar, u, v):
    """One power step: (u', v', sigma)."""
    W = w_bar.reshape(w_bar.shape[0], -1)
    v2 = l2n(W.t() @ u)
    Wv = W @ v2
    u2 = l2n(Wv)
    return u2, v2, u2 @ Wv


def lrelu(z):
    return torch.where(z > 0, z, z * SLOPE)


def lrelu_grad(a):
    """Derivative of the LeakyReLU that produced a (a and its pre-activation have the same sign)."""
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))


def conv4s2(x, w_bar, bias, sigma, act=True, defect=None):
    b = bias / sigma if defect == "sigma_bias" else bias
    z = F.conv2d(x, w_bar, None, 2, 1) / sigma + b.view(1, -1, 1, 1)
    return lrelu(z) if act else z


def conv4s2_dgrad(dz, w_bar, sigma, in_hw, defect=None):
    """Gather form: input row iy = py + 2a takes filter rows ky = 1 - py + 2 ty from output rows oy = a + py - ty."""
    (N, Cout, OH, OW), Cin, (H, W) = dz.shape, w_bar.shape[1], in_hw
    dx = dz.new_zeros((N, Cin, H, W))
    for py in range(2):
        for px in range(2):
            sub = dx[:, :, py::2, px::2]
            HA, WB = sub.shape[2:]
            for ty in range(2):
                for tx in range(2):
                    ky = (py if defect == "parity" else 1 - py) + 2 * ty
                    kx = 1 - px + 2 * tx
                    a0, a1 = max(0, ty - py), min(HA, OH + ty - py)     # 0 <= a + py - ty < OH
                    b0, b1 = max(0, tx - px), min(WB, OW + tx - px)
                    if a1 <= a0 or b1 <= b0:
                        continue
                    z = dz[:, :, a0 + py - ty:a1 + py - ty, b0 + px - tx:b1 + px - tx]
                    sub[:, :, a0:a1, b0:b1] += torch.einsum("nohw,oc->nchw", z, w_bar[:, :, ky, kx])
    return dx / sigma


def last_fwd(x, w_bar, bias, sigma, defect=None):
    N, C, H, W = x.shape
    cnt = 18 if defect == "mean" else (H - 2) * (W - 5)
    return (F.conv2d(x, w_bar).sum((2, 3)) / sigma / cnt + bias.view(1, 1)).view(N, 1)


def last_bwd(g, w_bar, sigma, x_shape):
    N, C, H, W = x_shape
    OH, OW = H - 2, W - 5
    dx = g.new_zeros(x_shape)
    for ky in range(3):
        for kx in range(6):
            dx[:, :, ky:ky + OH, kx:kx + OW] += w_bar[0, :, ky, kx].view(1, C, 1, 1)
    return dx * (g.view(N, 1, 1, 1) / sigma / (OH * OW))


def softmax_rows(e):
    p = torch.exp(e - e.max(-1, keepdim=True).values)
    return p / p.sum(-1, keepdim=True)


def softmax_rows_bwd(a, dA, defect=None):
    if defect == "softmax_sum":
        return a * dA
    return a * (dA - (a * dA).sum(-1, keepdim=True))


def attention_core(q, k, v):
    """q, k, v [N, C, P] -> (o [N, C, P], a [N, P, P])."""
    a = softmax_rows(q.transpose(1, 2) @ k)
    return v @ a.transpose(1, 2), a


def attention_core_bwd(q, k, v, a, do, defect=None):
    dv = do @ a
    dE = softmax_rows_bwd(a, do.transpose(1, 2) @ v, defect)
    return k @ dE.transpose(1, 2), q @ dE, dv          # dq, dk, dv


def attention(x, ws, bs, sigmas, gamma):
    """ws / bs / sigmas: the three 1x1 projections (query, key, value).  Returns (y, cache)."""
    N, C, h, w = x.shape
    xf = x.reshape(N, C, h * w)
    q, k, v = ((W.reshape(C, C) / s) @ xf + b.view(1, C, 1) for W, b, s in zip(ws, bs, sigmas))
    o, a = attention_core(q, k, v)
    return (gamma * o + xf).view(N, C, h, w), (q, k, v, a)


def attention_bwd(cache, ws, sigmas, gamma, dy, defect=None):
    q, k, v, a = cache
    N, C, h, w = dy.shape
    dyf = dy.reshape(N, C, h * w)
    dx = dyf.clone()
    for W, s, d in zip(ws, sigmas, attention_core_bwd(q, k, v, a, gamma * dyf, defect)):
        dx = dx + (W.reshape(C, C) / s).t() @ d
    return dx.view(N, C, h, w)


def _sn(sd, prefix, dtype):
    return tuple(sd[f"{prefix}.{n}"].to(dtype) for n in ("weight_bar", "bias", "weight_u", "weight_v"))


def forward(sd, x, dtype=torch.float64, defect=None):
    """(output [N, 1], feature4, cache); cache["uv"][prefix] = the updated (u, v)."""
    x = x.to(dtype)
    c = {"x_shape": x.shape, "act": [None], "sigma": [None], "w": [None], "uv": {}}
    a = x
    for name in LAYERS:
        w, b, u, v = _sn(sd, name + ".0.module", dtype)
        u, v, s = sigma_step(w, u, v)
        c["uv"][name + ".0.module"] = (u, v)
        a = conv4s2(a, w, b, s, defect=defect)
        c["act"].append(a), c["sigma"].append(s), c["w"].append(w)
        if name == "layer4":
            ws, bs, ss = [], [], []
            for conv in ATT:
                w, b, u, v = _sn(sd, f"attention.{conv}.module", dtype)
                u, v, s = sigma_step(w, u, v)
                c["uv"][f"attention.{conv}.module"] = (u, v)
                ws.append(w), bs.append(b), ss.append(s)
            c["att_w"], c["att_s"], c["gamma"] = ws, ss, sd["attention.gamma"].to(dtype)
            a, c["att"] = attention(a, ws, bs, ss, c["gamma"])
    w, b, u, v = _sn(sd, "last.module", dtype)
    u, v, s = sigma_step(w, u, v)
    c["uv"]["last.module"] = (u, v)
    c["w_last"], c["s_last"] = w, s
    return last_fwd(a, w, b, s, defect), c["act"][4], c


def backward(c, g_out=None, g_f4=None, defect=None):
    """d loss / d x for the gradients at the two outputs (either may be None)."""
    act, sig, w = c["act"], c["sigma"], c["w"]
    dt = act[1].dtype
    d4 = None
    if g_out is not None:
        d = last_bwd(g_out.to(dt), c["w_last"], c["s_last"], act[6].shape) * lrelu_grad(act[6])
        d = conv4s2_dgrad(d, w[6], sig[6], act[5].shape[2:], defect) * lrelu_grad(act[5])
        d = conv4s2_dgrad(d, w[5], sig[5], act[4].shape[2:], defect)
        d4 = attention_bwd(c["att"], c["att_w"], c["att_s"], c["gamma"], d, defect)
    if g_f4 is not None:
        d4 = g_f4.to(dt) if d4 is None else d4 + g_f4.to(dt)
    d = d4 * lrelu_grad(act[4])
    for i in (4, 3, 2):
        d = conv4s2_dgrad(d, w[i], sig[i], act[i - 1].shape[2:], defect) * lrelu_grad(act[i - 1])
    return conv4s2_dgrad(d, w[1], sig[1], c["x_shape"][2:], defect)


def autograd_composition(sd, x, g_out=None, g_f4=None):
    """The same network from nn.Conv2d modules and torch.softmax under float64 autograd, sigma from the same power step (a
    constant: the critic is frozen).  Returns (output, feature4, dx)."""
    dt = torch.float64
    x = x.to(dt).clone().requires_grad_(True)

    def conv(prefix, stride, pad):
        w, b, u, v = _sn(sd, prefix, dt)
        m = torch.nn.Conv2d(w.shape[1], w.shape[0], tuple(w.shape[2:]), stride, pad).to(dt)
        with torch.no_grad():
            m.weight.copy_(w / sigma_step(w, u, v)[2])
            m.bias.copy_(b)
        return m

    a = x
    for name in LAYERS:
        a = F.leaky_relu(conv(name + ".0.module", 2, 1)(a), SLOPE)
        if name == "layer4":
            f4 = a
            N, C, h, w = a.shape
            q, k, v = (conv(f"attention.{n}.module", 1, 0)(a).view(N, C, h * w) for n in ATT)
            att = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=-1)
            a = sd["attention.gamma"].to(dt) * torch.bmm(v, att.transpose(1, 2)).view(N, C, h, w) + a
    out = conv("last.module", 1, 0)(a).mean((2, 3)).view(-1, 1)
    loss = 0
    if g_out is not None:
        loss = loss + (out * g_out.to(dt)).sum()
    if g_f4 is not None:
        loss = loss + (f4 * g_f4.to(dt)).sum()
    loss.backward()
    return out.detach(), f4.detach(), x.grad


def attention_inputs(C, P, seed=0, peak=None, N=2):
    """float32 (q, k, v, do) [N, C, P] whose energies sum_c q k have standard deviation 3 — O(1-10), so that float32 softmax
    arithmetic stays within 1e-4 of float64 (tests/test_gan_host.py asserts it).  peak: channel 0 carries sqrt(peak) in every
    query and in ONE key (column P // 2), so every row's maximum is near `peak` and far above the rest of its row."""
    g = torch.Generator().manual_seed(1000 * C + P + seed)
    scale = (3.0 / C ** 0.5) ** 0.5
    q, k = (torch.randn(N, C, P, generator=g) * scale for _ in range(2))
    v, do = (torch.randn(N, C, P, generator=g) for _ in range(2))
    if peak is not None:
        q[:, 0, :] = peak ** 0.5
        k[:, 0, :] = 0
        k[:, 0, P // 2] = peak ** 0.5
    return q, k, v, do


ATTENTION_CASES = [(8, 1, None), (8, 7, None), (8, 33, None), (8, 312, None), (256, 312, None), (8, 33, 200.0)]
