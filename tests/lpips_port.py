"""LPIPS v0.1 (net='alex', lpips=True, spatial=False, eval mode) as torch.nn.functional calls: the test-side yardstick, written from
the definition (the published package is on none of the test machines).  dtype-generic: the state and the images are cast to `dtype`
(fp64: the reference; fp32: its own rounding error, the e32 of the tests' bar)."""
import torch
import torch.nn.functional as F

CONV = (("net.slice1.0", 4, 2), ("net.slice2.3", 1, 2), ("net.slice3.6", 1, 1), ("net.slice4.8", 1, 1), ("net.slice5.10", 1, 1))


def features(state, x, dtype):
    """The five post-ReLU feature maps [N,C_l,H_l,W_l] of x [N,3,H,W] (already in the network's input range)."""
    sd = {k: v.to(dtype) for k, v in state.items()}
    h = (x.to(dtype) - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    feats = []
    for i, (key, stride, pad) in enumerate(CONV):
        if i in (1, 2):
            h = F.max_pool2d(h, kernel_size=3, stride=2)
        h = F.relu(F.conv2d(h, sd[key + ".weight"], sd[key + ".bias"], stride=stride, padding=pad))
        feats.append(h)
    return feats


def _normalize(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def lpips(state, in0, in1, dtype=torch.float64, normalize=False):
    """-> (value [N,1,1,1], layers [N,5], feats0, feats1) in `dtype`."""
    in0, in1 = in0.to(dtype), in1.to(dtype)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    f0, f1 = features(state, in0, dtype), features(state, in1, dtype)
    layers = []
    for l in range(5):
        diff = (_normalize(f0[l]) - _normalize(f1[l])) ** 2
        d = F.conv2d(diff, state[f"lin{l}.model.1.weight"].to(dtype))          # [N,1,H,W]; the Dropout before it is the identity in eval
        layers.append(d.mean(dim=(2, 3), keepdim=True))
    val = layers[0]
    for l in range(1, 5):
        val = val + layers[l]
    return val, torch.cat([d.reshape(-1, 1) for d in layers], dim=1), f0, f1


def zero_pixel_share(feat):
    """The share of pixels of a feature map [N,C,H,W] whose channels are all zero."""
    return float((feat.abs().amax(dim=1) == 0).double().mean())
