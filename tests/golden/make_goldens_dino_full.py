"""Writes the fixtures of DINO's full-image path from the REAL reference:  python tests/golden/make_goldens_dino_full.py /path/to/NeRF-SOS

What engines/eval.py:133-137 (and :237-241) feeds the network: the rendered rgb through normalize_batch, then
VitExtractor.get_vit_attn_feat_noresize (models/extractor.py:215-224: normalised again, no resize) on the reference's
vit_small(patch_size=16) (models/vision_transformer.py, position embedding interpolated by interpolate_pos_encoding).  The model is
built and hooked exactly as tests/golden/make_goldens_dino.py does, with the weights of tests/dino_weights.py.  The port
(tests/dino_full_port.py) is asserted bit-identical to the reference on CPU in fp32 before anything is written, and every case
and output must satisfy 4 * e32 <= 1e-4 * scale (e32 = the reference's own fp32 distance from its fp64 run, scale = max |fp64|).

The inputs are NOT stored (a 756 x 1008 image is 9 MB): they are `default_rng(seed).random((B, H, W, 3), float32)`, and the sha256 of
each is recorded.  Files (all under tests/golden/, each under 1 MiB):
  dino_full.npz            `meta`: JSON -- seeds, state sha256 per weight kind, the case table (kind, h, w, B, seed, rows, cols,
                           feat_stride, input_sha256)
  dino_full_c<i>.npz       case i: the reference's fp32 `attn32` [B,1,rows*cols] / `cls32` [B,384] and fp64 `attn64` / `cls64`, `e32`
                           and `scale` per output (attn, cls_, feat; over every element of every image)
  dino_full_feat32_c<i>.npz fp32 feat rows 0, s, 2s, .. (s = feat_stride) of every image, [B, ceil(rows*cols / s), 384]
  dino_full_feat64_c<i>.npz fp64 feat rows of image 0 at the same stride
"""
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dino_full_port as port     # noqa: E402
import dino_weights as dw         # noqa: E402
from helpers import state_sha     # noqa: E402
from make_goldens_dino import SEEDS, reference_run   # noqa: E402

CASES = [
    dict(kind="wide", h=756, w=1008, B=1, seed=201),    # flower eval size: 47 x 63 patches, 4 remainder rows
    dict(kind="init", h=756, w=1008, B=1, seed=202),
    dict(kind="init", h=800, w=800, B=1, seed=203),     # Blender: 50 x 50, 2 501 tokens
    dict(kind="peaky", h=224, w=224, B=1, seed=204),    # pos_embed as it is
    dict(kind="wide", h=232, w=232, B=1, seed=205),     # the short cut at a size that is not 224
    dict(kind="init", h=224, w=239, B=1, seed=206),     # 196 patches but H != W: interpolated at scale 14.1 / 14
    dict(kind="wide", h=100, w=130, B=1, seed=207),     # remainder in both dimensions
    dict(kind="peaky", h=48, w=1024, B=1, seed=208),    # 3 x 64
    dict(kind="init", h=64, w=80, B=2, seed=209),       # a batch
]
MAX_ROWS = 300       # stored feat rows per image: 300 * 384 * 8 B = 0.9 MB for the fp64 file


def make_input(case):
    return np.random.default_rng(case["seed"]).random((case["B"], case["h"], case["w"], 3), dtype=np.float32)


def input_sha(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype="<f4").tobytes()).hexdigest()


def main(ref_root):
    sys.path.insert(0, ref_root)
    sys.path.insert(0, os.path.join(ref_root, "models"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_vit", os.path.join(ref_root, "models", "vision_transformer.py"))
    vt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vt)

    states, models32, models64 = {}, {}, {}
    for kind, seed in SEEDS.items():
        states[kind] = dw.make_state(kind, seed)
        m = vt.vit_small(patch_size=16).eval()
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == dw.key_shapes(), "checkpoint contract"
        m.load_state_dict(states[kind])
        models32[kind] = m
        m64 = vt.vit_small(patch_size=16).eval().double()
        m64.load_state_dict({k: v.double() for k, v in states[kind].items()})
        models64[kind] = m64

    meta = {"state_sha256": {k: state_sha(states[k]) for k in SEEDS}, "seeds": SEEDS, "cases": []}
    for ci, case in enumerate(CASES):
        kind = case["kind"]
        rgb = make_input(case)
        x = torch.from_numpy(rgb)
        img = port.normalize(port.eval_dino_in(x))               # normalize_batch, then get_vit_attn_feat_noresize's own
        img64 = port.normalize(port.eval_dino_in(x.double()))
        ref = reference_run(models32[kind], img)
        mine = port.network(states[kind], img)
        for k in ("attn", "cls_", "feat"):
            assert torch.equal(ref[k], mine[k]), f"port differs from the reference: case {ci} {k}"
        ref64 = reference_run(models64[kind], img64)
        e32 = [float((ref[k].double() - ref64[k]).abs().max()) for k in ("attn", "cls_", "feat")]
        scale = [float(ref64[k].abs().max()) for k in ("attn", "cls_", "feat")]
        print(f"case {ci} {case}: e32 {e32} scale {scale} ratio {[e / s for e, s in zip(e32, scale)]}", flush=True)
        for e, sc in zip(e32, scale):
            assert 4.0 * e <= 1e-4 * sc, f"case {ci}: the reference's own fp32 error {e} is above 2.5e-5 of scale {sc}"
        rows, cols = port.grid_of(case["h"], case["w"])
        stride = math.ceil(rows * cols / MAX_ROWS)
        np.savez(os.path.join(HERE, f"dino_full_c{ci}.npz"), attn32=ref["attn"].numpy(), cls32=ref["cls_"].numpy(),
                 attn64=ref64["attn"].numpy(), cls64=ref64["cls_"].numpy(), e32=np.array(e32), scale=np.array(scale))
        np.savez(os.path.join(HERE, f"dino_full_feat32_c{ci}.npz"), feat=ref["feat"][:, ::stride].numpy())
        np.savez(os.path.join(HERE, f"dino_full_feat64_c{ci}.npz"), feat=ref64["feat"][0, ::stride].numpy())
        meta["cases"].append(dict(case, rows=rows, cols=cols, feat_stride=stride, input_sha256=input_sha(rgb)))
    np.savez(os.path.join(HERE, "dino_full.npz"), meta=np.array(json.dumps(meta)))
    for n in sorted(os.listdir(HERE)):
        if n.startswith("dino_full"):
            size = os.path.getsize(os.path.join(HERE, n))
            assert size < (1 << 20), (n, size)
            print(n, size)


if __name__ == "__main__":
    main(sys.argv[1])
