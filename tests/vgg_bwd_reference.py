"""Float64 CPU references for the input gradient of VGG19_pytorch (tests/test_gpu_vgg_backward.py).

`vgg_input_grad64(..., pins=None)` is plain float64 autograd through oracle.dvc_oracle.vgg19_forward.  With `pins` (key ->
the post-ReLU output R of that layer as the device computed it) the ReLU masks [R > 0] and the max-pool arg-maxes are
taken from those tensors instead of the float64 forward's own: the float64 gradient of the same piecewise-linear map the
device differentiates.  Without pins a pre-activation within fp32 rounding of 0, or two pool candidates within rounding of
each other, may fall on the other side in float64 and move a whole gradient entry; that is a property of the fp32 forward,
not of the backward under test.
"""
import torch
import torch.nn.functional as F

from oracle import dvc_oracle as O


def loss_grads(outs, seed):
    """Seeded G_k, one per output: the loss is sum_k <G_k, out_k>."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]


def vgg_forward64(sd64, x, out_keys, preprocess=True, pool="max", pins=None):
    last = max(O._VGG_SEQ.index(next(s for s in O._VGG_SEQ if s[0] == k)) for k in out_keys)
    out = {}
    cur = O.vgg_preprocess(x) if preprocess else x
    prev = None
    for i, (key, conv) in enumerate(O._VGG_SEQ):
        if i > last:
            break
        if conv is None:
            if pool == "max" and pins is not None:
                _, idx = F.max_pool2d(pins[prev], 2, 2, return_indices=True)
                cur = cur.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            else:
                cur = F.max_pool2d(cur, 2, 2) if pool == "max" else F.avg_pool2d(cur, 2, 2)
        else:
            z = F.conv2d(cur, sd64[conv + ".weight"], sd64[conv + ".bias"], padding=1)
            cur = z * (pins[key] > 0).to(z.dtype) if pins is not None else F.relu(z)
        out[key] = cur
        prev = key
    return [out[k] for k in out_keys]


def vgg_input_grad64(sd, x, out_keys, G, preprocess=True, pool="max", pins=None):
    """d/dx of sum_k <G_k, out_k> in float64 (G_k None: that output does not enter the loss)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    pins = None if pins is None else {k: v.double() for k, v in pins.items()}
    x = x.double().detach().requires_grad_(True)
    with torch.enable_grad():
        outs = vgg_forward64(sd64, x, out_keys, preprocess, pool, pins)
        loss = sum((o * g).sum() for o, g in zip(outs, G) if g is not None)
        loss.backward()
    return x.grad


def vgg_input_grad_f32(sd, x, out_keys, G, preprocess=True, pool="max"):
    """The same gradient by float32 CPU autograd through the oracle (the yardstick printed beside the device's error)."""
    sd32 = {k: v.float() for k, v in sd.items()}
    x = x.float().detach().requires_grad_(True)
    with torch.enable_grad():
        outs = O.vgg19_forward(sd32, x, out_keys, preprocess=preprocess, pool=pool)
        loss = sum((o * g.float()).sum() for o, g in zip(outs, G) if g is not None)
        loss.backward()
    return x.grad.double()


def rel_errors(got, ref):
    got, ref = got.double(), ref.double()
    rel_l2 = ((got - ref).norm() / ref.norm()).item()
    rel_max = ((got - ref).abs().max() / ref.abs().max()).item()
    return rel_l2, rel_max
