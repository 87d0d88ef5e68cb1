"""Cases and loader of the DINO backward fixtures written by tests/golden/make_goldens_dino_bwd.py (a plain helper, not a conftest).

The inputs and the upstream gradients are drawn here, by formula (numpy's PCG64, as tests/dino_weights.py draws the weights), by the
generator and by the tests alike; the fixture stores their sha256 and the reference's fp64 results.  Storing the draws themselves
would add 4.6 MB of noise to the repository, and the 250 x 230 input alone is two thirds of the size limit for a committed file."""
import hashlib
import json
import os

import numpy as np

import dino_fixture as fx

GOLDEN = fx.GOLDEN
CHUNK = 100_000          # fp64 values per gradient file: 0.8 MB
BLOCKS, BLOCK_ROWS = (11, 5, 0), 50
CASES = [   # mode "patch": rgb [B,P,P,3] + patch_stride (trainer steps 1-2); "extractor": [B,3,h,w]; "prepared": the network input itself
    dict(kind="init", mode="patch", P=32, stride=1, B=2, seed=201),        # 32 -> 224 up-sampling, 49 preimages per pixel
    dict(kind="wide", mode="patch", P=64, stride=6, B=2, seed=202),        # the shipped recipe's 384 -> 224
    dict(kind="peaky", mode="patch", P=48, stride=5, B=3, seed=203),       # 240 -> 224, odd batch, peaked softmax rows
    dict(kind="wide", mode="extractor", h=40, w=56, B=1, seed=204),        # not square, one normalisation
    dict(kind="init", mode="extractor", h=250, w=230, B=1, seed=205),      # pixels with no preimage: exact zeros
    dict(kind="peaky", mode="prepared", h=224, w=224, B=1, seed=206),      # embedding data gradient alone, factor 1
]
_cache = {}


def draws(case):
    """(input, g_feat [B,196,384], g_cls [B,384]) of a case, float32: the input uniform in [0, 1) (standard normal for a prepared
    one), the upstream gradients standard normal."""
    rng = np.random.default_rng(case["seed"])
    B = case["B"]
    if case["mode"] == "patch":
        x = rng.random((B, case["P"], case["P"], 3))
    elif case["mode"] == "extractor":
        x = rng.random((B, 3, case["h"], case["w"]))
    else:
        x = rng.standard_normal((B, 3, 224, 224))
    g_feat, g_cls = rng.standard_normal((B, 196, 384)), rng.standard_normal((B, 384))
    return x.astype(np.float32), g_feat.astype(np.float32), g_cls.astype(np.float32)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).astype("<f4").tobytes())
    return h.hexdigest()


def meta():
    if "meta" not in _cache:
        _cache["meta"] = json.loads(str(np.load(os.path.join(GOLDEN, "dino_bwd.npz"))["meta"]))
    return _cache["meta"]


def case(ci):
    """Case ci: the table entry, the draws (checked against the generator's sha256), the reference's fp64 input gradient `g64`
    (input's shape), `e32` = max |fp32 autograd - fp64 autograd| and `scale` = max |fp64|."""
    if ci not in _cache:
        m = meta()["cases"][ci]
        c = dict(CASES[ci])
        assert {k: m[k] for k in c} == c, "the case table differs from the generator's"
        x, g_feat, g_cls = draws(c)
        assert sha(x, g_feat, g_cls) == m["sha256"], f"case {ci}: the draws differ from the generator's"
        flat = np.concatenate([np.load(os.path.join(GOLDEN, f"dino_bwd_c{ci}_g{j}.npz"))["g64"] for j in range(m["chunks"])])
        c.update(input=x, g_feat=g_feat, g_cls=g_cls, g64=flat.reshape(x.shape), e32=float(m["e32"]), scale=float(m["scale"]))
        _cache[ci] = c
    return _cache[ci]


def block_grads():
    """Case 0: {block: (fp64 residual-stream gradient at the block's input, tokens 0..49 of image 0; its e32; its scale)}."""
    d = np.load(os.path.join(GOLDEN, "dino_bwd_blocks.npz"))
    return {k: (d[f"g64_{k}"], float(d[f"e32_{k}"]), float(d[f"scale_{k}"])) for k in BLOCKS}


def bar(e32, scale):
    """tests/dino_fixture.py::bar on one quantity: max(4 * e32, 1e-6 * scale), never above 1e-4 * scale."""
    return fx.bar({"e32": {"g": e32}, "scale": {"g": scale}}, "g")


def port_features(sd, x, c):
    """tests/dino_port.py on a case's input with autograd on: {'attn', 'cls_', 'feat'} in the dtype of x and sd."""
    import dino_port as port
    if c["mode"] == "patch":
        img = port.prepare(x, c["stride"])
    else:
        img = port.extractor_step2(x) if c["mode"] == "extractor" else x
    return port.network(sd, img)


def port_input_grad(sd, c, dtype, device="cpu"):
    """d (sum feat * g_feat + sum cls_ * g_cls) / d input by torch autograd through the port, in `dtype`."""
    import torch
    sd = {k: v.to(device, dtype) for k, v in sd.items()}
    x = torch.from_numpy(c["input"]).to(device, dtype).requires_grad_()
    out = port_features(sd, x, c)
    loss = (out["feat"] * torch.from_numpy(c["g_feat"]).to(device, dtype)).sum() + (out["cls_"] * torch.from_numpy(c["g_cls"]).to(device, dtype)).sum()
    return torch.autograd.grad(loss, x)[0]
