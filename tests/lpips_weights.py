"""LPIPS (AlexNet) state dicts by formula (a plain helper, not a conftest).  The real weights (torchvision's AlexNet, the lpips
package's alex.pth) are on none of the test machines, so the tests build the 17 tensors from numpy's PCG64 (`default_rng(seed)`),
drawing in SORTED key order.  tests/golden/lpips.npz stores the sha256 of each generated state."""
import hashlib

import numpy as np
import torch

CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))
CHANNELS = (64, 192, 384, 256, 256)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
KINDS = ("he", "wide", "sparse")
SPARSE_BIAS_SHIFT = {"net.slice3.6.bias": -80.0, "net.slice5.10.bias": -9.0}   # layers 2 and 4


def key_shapes():
    """The checkpoint contract: names and shapes of lpips.LPIPS(net='alex').state_dict() (without its duplicate `lins.*`)."""
    out = [("scaling_layer.shift", (1, 3, 1, 1)), ("scaling_layer.scale", (1, 3, 1, 1))]
    for key, shp in zip(CONV_KEYS, CONV_SHAPES):
        out += [(key + ".weight", shp), (key + ".bias", (shp[0],))]
    out += [(f"lin{i}.model.1.weight", (1, c, 1, 1)) for i, c in enumerate(CHANNELS)]
    return out


def make_state(kind, seed):
    """kind:
    "he"      conv weights N(0, 2 / fan_in), biases 0, lin = |N(0, 1)| (non-negative, as in the trained model);
    "wide"    conv weights x2, biases N(0, 0.2);
    "sparse"  "wide" with the biases of layers 2 and 4 shifted negative (SPARSE_BIAS_SHIFT), so that at those layers some pixels
              have EVERY channel at zero: the 0 / (0 + 1e-10) path of the normalisation.
    The scaling layer keeps its constants.  Draw order: sorted keys; per key one standard_normal block of the tensor's size."""
    assert kind in KINDS, kind
    rng = np.random.default_rng(seed)
    shapes = dict(key_shapes())
    sd = {}
    for k in sorted(shapes):
        shp = shapes[k]
        z = rng.standard_normal(shp)
        if k == "scaling_layer.shift":
            v = np.array(SHIFT).reshape(shp)
        elif k == "scaling_layer.scale":
            v = np.array(SCALE).reshape(shp)
        elif k.startswith("lin"):
            v = np.abs(z)
        elif k.endswith("bias"):
            v = np.zeros(shp) if kind == "he" else 0.2 * z
            if kind == "sparse":
                v = v + SPARSE_BIAS_SHIFT.get(k, 0.0)
        else:
            fan_in = shp[1] * shp[2] * shp[3]
            v = z * np.sqrt(2.0 / fan_in) * (1.0 if kind == "he" else 2.0)
        sd[k] = torch.from_numpy(np.ascontiguousarray(v.astype(np.float32)))
    return {k: sd[k] for k, _ in key_shapes()}     # the module's own key order


def state_sha256(sd):
    h = hashlib.sha256()
    for k, _ in key_shapes():
        h.update(k.encode() + b"\0" + sd[k].numpy().tobytes())
    return h.hexdigest()


# ---- the test cases: (name, N, H, W, noise sigma, weight kinds), seeds by position
CASES = (("min31", 1, 31, 31, 0.1, ("he", "wide")),
         ("odd33x47", 2, 33, 47, 0.3, ("he", "wide")),
         ("patch64", 1, 64, 64, 0.02, ("he", "wide", "sparse")),
         ("rows713", 1, 97, 130, 0.05, ("he", "wide", "sparse")))
STATE_SEEDS = {"he": 11, "wide": 12, "sparse": 13}


def make_images(index):
    """Uniform [0,1] images; the second is the first plus Gaussian noise, clipped to [0,1].  fp32 [N,3,H,W] numpy arrays."""
    _, n, h, w, sigma, _ = CASES[index]
    rng = np.random.default_rng(1000 + index)
    a = rng.uniform(0.0, 1.0, (n, 3, h, w))
    b = np.clip(a + sigma * rng.standard_normal((n, 3, h, w)), 0.0, 1.0)
    return a.astype(np.float32), b.astype(np.float32)
