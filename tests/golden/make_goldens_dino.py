"""Writes the DINO ViT-S/16 fixtures from the REAL reference:  python tests/golden/make_goldens_dino.py /path/to/NeRF-SOS

The reference's vit_small(patch_size=16) (models/vision_transformer.py) is built without network access and given the weights of
tests/dino_weights.py; the two hooks of VitExtractor.get_feat_attn_from_input (models/extractor.py:49-58,109-117) are replicated
here, because VitExtractor.__init__ itself calls torch.hub.  The port (tests/dino_port.py) is asserted bit-identical to the
reference on CPU in fp32 before anything is written.

Data only, every file under 1 MiB, hence several files (all under tests/golden/):
  dino_vit.npz            `meta`: JSON -- the checkpoint's key / shape list, the sha256 of every generated state, the case table,
                          which image sits where in the feat32 chunks
  dino_vit_c<i>.npz       case i: `input` (rgb [B,P,P,3] as rendered, or the extractor's [B,3,h,w]), the reference's fp32 `attn32` /
                          `cls32`, the same from an fp64 run of the reference module with the same weights (`attn64` / `cls64`, all
                          images), `e32` = max |fp32 - fp64| and `scale` = max |fp64| per output (attn, cls_, feat; over ALL images of
                          the case), `argmin` of the fp64 similarity matrix of cls_ and its top-two `gap`
  dino_vit_feat32_<j>.npz the reference's fp32 `feat` of three images each (every image of every case)
  dino_vit_feat64_c<i>.npz the fp64 `feat` of image 0 of case i (the other images are compared against fp32 at 2 x the bar)
  dino_vit_prepared.npz   the network input [3,224,224] of one image of the P = 48, stride 5 case (240 -> 224: the nearest-index rule)
  dino_vit_block<k>.npz   fp64 output of block k (0 and 5; block 11 is cls_ / feat), tokens 0..49 of image 0 of case 0, with its e32
Total: about 11.5 MB in 22 files.  The 16 images' fp32 feat alone is 4.8 MB and the six fp64 feat 3.6 MB, so one file under the
largest existing fixture (5.7 MB) was not possible with these cases; every file stays under the 1 MiB limit for a committed file.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dino_port as port          # noqa: E402
import dino_weights as dw         # noqa: E402
from helpers import state_sha     # noqa: E402

SEEDS = {"wide": 11, "init": 12, "peaky": 13}
CASES = [   # mode "patch": rgb [B,P,P,3] + patch_stride (trainer steps 1-2); "extractor": [B,3,h,w] through get_vit_attn_feat alone
    dict(kind="wide", mode="patch", P=64, stride=6, B=8, seed=101),        # the shipped recipe (scripts/train_flower_node0.sh)
    dict(kind="init", mode="patch", P=32, stride=1, B=2, seed=102),
    dict(kind="peaky", mode="patch", P=48, stride=5, B=3, seed=103),       # 240 -> 224
    dict(kind="peaky", mode="extractor", h=224, w=224, B=1, seed=104),     # already 224: the resize is the identity
    dict(kind="wide", mode="extractor", h=40, w=56, B=1, seed=105),        # not square
    dict(kind="init", mode="patch", P=64, stride=6, B=1, seed=106),        # 384 -> 224
]
CHUNK = 3
BLOCK_ROWS = 50      # tokens 0..49 of the block checkpoints (the class token and 3.5 rows of patches)
GAP_BAR = 1e-4


def make_input(case):
    rng = np.random.default_rng(case["seed"])
    if case["mode"] == "patch":
        return rng.random((case["B"], case["P"], case["P"], 3)).astype(np.float32)
    return rng.random((case["B"], 3, case["h"], case["w"])).astype(np.float32)


def reference_run(model, img):
    """get_feat_attn_from_input + the tail of get_vit_attn_feat, with every block's output on the side."""
    blocks, attn = [], []
    hooks = [b.register_forward_hook(lambda m, i, o: blocks.append(o)) for b in model.blocks]
    hooks.append(model.blocks[-1].attn.attn_drop.register_forward_hook(lambda m, i, o: attn.append(o)))
    with torch.no_grad():
        model(img)
    for h in hooks:
        h.remove()
    return {"attn": attn[-1].mean(1).unsqueeze(1)[:, :, 0, 1:], "cls_": blocks[-1][:, 0, :], "feat": blocks[-1][:, 1:, :], "blocks": blocks}


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

    meta = {"keys": [[k, list(s)] for k, s in dw.key_shapes()], "state_sha256": {k: state_sha(states[k]) for k in SEEDS},
            "seeds": SEEDS, "cases": [], "chunk": CHUNK, "gap_bar": GAP_BAR}
    feats32 = []
    for ci, case in enumerate(CASES):
        kind = case["kind"]
        x = torch.from_numpy(make_input(case))
        if case["mode"] == "patch":
            img = port.prepare(x, case["stride"])
            img64 = port.prepare(x.double(), case["stride"])
        else:
            img = port.extractor_step2(x)
            img64 = port.extractor_step2(x.double())
        ref = reference_run(models32[kind], img)
        mine = port.network(states[kind], img, want_blocks=True)
        for k in ("attn", "cls_", "feat"):
            assert torch.equal(ref[k], mine[k]), f"port differs from the reference: case {ci} {k}"
        for a, b in zip(ref["blocks"], mine["blocks"]):
            assert torch.equal(a, b)
        ref64 = reference_run(models64[kind], img64)
        e32 = [float((ref[k].double() - ref64[k]).abs().max()) for k in ("attn", "cls_", "feat")]
        scale = [float(ref64[k].abs().max()) for k in ("attn", "cls_", "feat")]
        for e, sc in zip(e32, scale):      # the fp32 bar 4 * e32 must stay under the project's end-to-end bar of 1e-4 * scale
            assert 4.0 * e <= 1e-4 * sc, f"case {ci}: the reference's own fp32 error {e} is above 2.5e-5 of scale {sc}"
        sim64, amin = port.similarity_argmin(ref64["cls_"])
        gap = -1.0
        if case["B"] >= 2:
            top2 = torch.sort(sim64, dim=0)[0][:2]
            gap = float((top2[1] - top2[0]).min())
            assert gap > GAP_BAR, f"case {ci}: top-two gap {gap}"
        np.savez(os.path.join(HERE, f"dino_vit_c{ci}.npz"), input=x.numpy(), attn32=ref["attn"].numpy(), cls32=ref["cls_"].numpy(),
                 attn64=ref64["attn"].numpy(), cls64=ref64["cls_"].numpy(), e32=np.array(e32), scale=np.array(scale),
                 argmin=amin.numpy().astype(np.int64), gap=np.array(gap))
        np.savez(os.path.join(HERE, f"dino_vit_feat64_c{ci}.npz"), feat=ref64["feat"][0].numpy())
        case = dict(case, first_image=len(feats32))
        feats32 += [ref["feat"][b].numpy() for b in range(case["B"])]
        meta["cases"].append(case)
        print(f"case {ci} {case}: e32 {e32} scale {scale} gap {gap}")
        if ci == 2:
            np.savez(os.path.join(HERE, "dino_vit_prepared.npz"), image=img[1].numpy(), case=np.array(ci), index=np.array(1))
        if ci == 0:
            for k in (0, 5):
                b32, b64 = ref["blocks"][k][0], ref64["blocks"][k][0]
                np.savez(os.path.join(HERE, f"dino_vit_block{k}.npz"), out64=b64[:BLOCK_ROWS].numpy(),
                         e32=np.array(float((ref["blocks"][k].double() - ref64["blocks"][k]).abs().max())))
                print(f"  block {k}: scale {float(b64.abs().max()):.3f} e32 {float((b32.double() - b64).abs().max()):.3e}")
    for j in range(0, len(feats32), CHUNK):
        np.savez(os.path.join(HERE, f"dino_vit_feat32_{j // CHUNK}.npz"), feat=np.stack(feats32[j:j + CHUNK]))
    meta["n_images"] = len(feats32)
    np.savez(os.path.join(HERE, "dino_vit.npz"), meta=np.array(json.dumps(meta)))
    for n in sorted(os.listdir(HERE)):
        if n.startswith("dino_vit"):
            size = os.path.getsize(os.path.join(HERE, n))
            assert size < (1 << 20), (n, size)
            print(n, size)


if __name__ == "__main__":
    main(sys.argv[1])
