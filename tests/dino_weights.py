"""DINO ViT-S/16 state dicts by formula (a plain helper, not a conftest).  The real checkpoint is 87 MB and on none of the test
machines, so the tests build the 150 tensors from numpy's PCG64 (`default_rng(seed)`, identical on every platform and numpy
version in use), drawing in SORTED key order.  tests/golden/dino_vit.npz stores the sha256 of each generated state."""
import numpy as np
import torch

DEPTH, WIDTH, TOKENS, HIDDEN = 12, 384, 197, 1536


def key_shapes():
    """The checkpoint contract: names and shapes of vit_small(patch_size=16).state_dict(), in the module's own order."""
    out = [("cls_token", (1, 1, WIDTH)), ("pos_embed", (1, TOKENS, WIDTH)), ("patch_embed.proj.weight", (WIDTH, 3, 16, 16)),
           ("patch_embed.proj.bias", (WIDTH,))]
    for i in range(DEPTH):
        b = f"blocks.{i}."
        out += [(b + "norm1.weight", (WIDTH,)), (b + "norm1.bias", (WIDTH,)), (b + "attn.qkv.weight", (3 * WIDTH, WIDTH)),
                (b + "attn.qkv.bias", (3 * WIDTH,)), (b + "attn.proj.weight", (WIDTH, WIDTH)), (b + "attn.proj.bias", (WIDTH,)),
                (b + "norm2.weight", (WIDTH,)), (b + "norm2.bias", (WIDTH,)), (b + "mlp.fc1.weight", (HIDDEN, WIDTH)),
                (b + "mlp.fc1.bias", (HIDDEN,)), (b + "mlp.fc2.weight", (WIDTH, HIDDEN)), (b + "mlp.fc2.bias", (WIDTH,))]
    out += [("norm.weight", (WIDTH,)), ("norm.bias", (WIDTH,))]
    return out


KINDS = ("init", "wide", "peaky")
PEAKY_GAIN_BLOCKS = ("blocks.1.norm2.", "blocks.5.norm2.", "blocks.9.norm2.")


def make_state(kind, seed):
    """kind:
    "init"  DINO's own init statistics: N(0, 0.02) clipped at two sigma for cls_token, pos_embed and every matrix (the patch
            convolution too), biases 0, LayerNorm 1 / 0;
    "wide"  matrices N(0, 0.06) clipped at two sigma (x3), every bias (LayerNorm's too) N(0, 0.1), LayerNorm gains 1 + N(0, 0.1):
            block outputs reach a few tens;
    "peaky" "wide", then the q and k rows of every qkv matrix x1.5 (on top of x3: sharply peaked softmax rows) and, in norm2 of
            blocks 1, 5 and 9, 4 channels drawn without replacement get gains uniform in [10, 50] (12 outlier gains in all, imitating
            the outlier channels of trained ViTs).  Outlier gains in every LayerNorm (norm1 feeds q and k) make the network chaotic: the
            reference's own fp32 run then sits 2e-4 of scale from its fp64 run and no fp32 bar means anything; with this recipe it
            stays below 1e-5 of scale (the generator asserts 4 * e32 <= 1e-4 * scale for every case).
    Draw order: sorted keys; per key one standard_normal block of the tensor's size (LayerNorm gains of "peaky": then choice, then
    uniform)."""
    assert kind in KINDS, kind
    rng = np.random.default_rng(seed)
    shapes = dict(key_shapes())
    sd = {}
    for k in sorted(shapes):
        shp = shapes[k]
        z = rng.standard_normal(shp)
        is_norm = ".norm" in k or k.startswith("norm.")
        if is_norm and k.endswith("weight"):
            v = np.ones(shp) if kind == "init" else 1.0 + 0.1 * z
            if kind == "peaky" and k.startswith(PEAKY_GAIN_BLOCKS):
                ch = rng.choice(WIDTH, size=4, replace=False)
                v[ch] = rng.uniform(10.0, 50.0, size=4)
        elif k.endswith("bias"):
            v = np.zeros(shp) if kind == "init" else 0.1 * z
        else:
            sigma = 0.02 if kind == "init" else 0.06
            v = np.clip(z, -2.0, 2.0) * sigma
            if kind == "peaky" and k.endswith("attn.qkv.weight"):
                v[:2 * WIDTH] *= 1.5
        sd[k] = torch.from_numpy(np.ascontiguousarray(v.astype(np.float32)))
    return {k: sd[k] for k, _ in key_shapes()}     # the module's own key order
