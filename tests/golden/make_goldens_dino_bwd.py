"""Writes the fixtures of DINO's backward to the input from the REAL reference:  python tests/golden/make_goldens_dino_bwd.py /path/to/NeRF-SOS

The reference's vit_small(patch_size=16) (models/vision_transformer.py) is built as tests/golden/make_goldens_dino.py builds it, with
the weights of tests/dino_weights.py.  Per case of tests/dino_bwd_fixture.py::CASES: the gradient of sum(feat * g_feat) + sum(cls_ *
g_cls) with respect to the input (the rendered patches, the extractor's image, or the prepared network input) by torch autograd through
the reference module in fp64 and in fp32; e32 = max |fp32 - fp64|, scale = max |fp64|.  The port (tests/dino_port.py) in fp64 is
asserted equal to the reference module to rounding before anything is written: the GPU machine has only the port.

Data only, every file under 1 MiB (all under tests/golden/):
  dino_bwd.npz             `meta`: JSON -- the case table with, per case, sha256 of the draws (input, g_feat, g_cls), e32, scale,
                           the number of gradient chunks
  dino_bwd_c<i>_g<j>.npz   `g64`: values j * 100000 .. of the flattened fp64 input gradient of case i
  dino_bwd_blocks.npz      case 0: the fp64 residual-stream gradient at the input of blocks 11, 5 and 0, tokens 0..49 of image 0
                           (`g64_<k>`), with `e32_<k>` and `scale_<k>` over the whole tensor
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dino_bwd_fixture as bfx    # noqa: E402
import dino_port as port          # noqa: E402
import dino_weights as dw         # noqa: E402

SEEDS = {"wide": 11, "init": 12, "peaky": 13}      # tests/golden/make_goldens_dino.py: the states whose sha256 dino_vit.npz pins


def reference_grads(model, c, dtype, blocks=()):
    """Autograd through the reference module: the input gradient and the gradient at the input of each block of `blocks`."""
    x = torch.from_numpy(c["input"]).to(dtype).requires_grad_()
    if c["mode"] == "patch":
        img = port.prepare(x, c["stride"])
    else:
        img = port.extractor_step2(x) if c["mode"] == "extractor" else x
    outs, ins = [], {}
    hooks = [model.blocks[-1].register_forward_hook(lambda m, i, o: outs.append(o))]
    for k in blocks:
        def keep(m, i, k=k):
            i[0].retain_grad()
            ins[k] = i[0]
        hooks.append(model.blocks[k].register_forward_pre_hook(keep))
    model(img)
    for h in hooks:
        h.remove()
    y = outs[-1]                          # block 11's output before the final norm (models/extractor.py:109-117)
    loss = (y[:, 1:, :] * torch.from_numpy(c["g_feat"]).to(dtype)).sum() + (y[:, 0, :] * torch.from_numpy(c["g_cls"]).to(dtype)).sum()
    loss.backward()
    return x.grad.detach(), {k: ins[k].grad.detach() for k in blocks}


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
        models32[kind] = vt.vit_small(patch_size=16).eval()
        models32[kind].load_state_dict(states[kind])
        models64[kind] = vt.vit_small(patch_size=16).eval().double()
        models64[kind].load_state_dict({k: v.double() for k, v in states[kind].items()})
        for m in (models32[kind], models64[kind]):
            for p in m.parameters():
                p.requires_grad_(False)

    meta = {"seeds": SEEDS, "cases": [], "chunk": bfx.CHUNK, "blocks": list(bfx.BLOCKS), "block_rows": bfx.BLOCK_ROWS}
    for ci, case in enumerate(bfx.CASES):
        c = dict(case)
        c["input"], c["g_feat"], c["g_cls"] = bfx.draws(case)
        blocks = bfx.BLOCKS if ci == 0 else ()
        g64, b64 = reference_grads(models64[c["kind"]], c, torch.float64, blocks)
        g32, b32 = reference_grads(models32[c["kind"]], c, torch.float32, blocks)
        p64 = bfx.port_input_grad(states[c["kind"]], c, torch.float64)
        scale = float(g64.abs().max())
        e_port = float((p64 - g64).abs().max())
        assert e_port <= 1e-10 * scale, f"case {ci}: the port's fp64 gradient is {e_port} from the reference module's (scale {scale})"
        e32 = float((g32.double() - g64).abs().max())
        assert 4.0 * e32 <= 1e-4 * scale, f"case {ci}: the reference's own fp32 error {e32} is above 2.5e-5 of scale {scale}"
        if case["mode"] == "extractor" and max(case["h"], case["w"]) > 224:
            assert int((g64 == 0).sum()) > 0, "pixels without a preimage have a zero gradient"
        flat = g64.numpy().reshape(-1)
        chunks = (flat.size + bfx.CHUNK - 1) // bfx.CHUNK
        for j in range(chunks):
            np.savez(os.path.join(HERE, f"dino_bwd_c{ci}_g{j}.npz"), g64=flat[j * bfx.CHUNK:(j + 1) * bfx.CHUNK])
        meta["cases"].append(dict(case, sha256=bfx.sha(c["input"], c["g_feat"], c["g_cls"]), e32=e32, scale=scale, chunks=chunks))
        print(f"case {ci} {case}: e32 {e32:.3e} scale {scale:.3e} e32/scale {e32 / scale:.2e} |port64 - ref64| {e_port:.1e}")
        if ci == 0:
            out = {}
            for k in bfx.BLOCKS:
                out[f"g64_{k}"] = b64[k][0, :bfx.BLOCK_ROWS].numpy()
                out[f"e32_{k}"] = np.array(float((b32[k].double() - b64[k]).abs().max()))
                out[f"scale_{k}"] = np.array(float(b64[k].abs().max()))
                print(f"  block {k}: scale {float(out[f'scale_{k}']):.3e} e32 {float(out[f'e32_{k}']):.3e}")
                assert 4.0 * float(out[f"e32_{k}"]) <= 1e-4 * float(out[f"scale_{k}"])
            np.savez(os.path.join(HERE, "dino_bwd_blocks.npz"), **out)
    np.savez(os.path.join(HERE, "dino_bwd.npz"), meta=np.array(json.dumps(meta)))
    for n in sorted(os.listdir(HERE)):
        if n.startswith("dino_bwd"):
            size = os.path.getsize(os.path.join(HERE, n))
            assert size < (1 << 20), (n, size)
            print(n, size)


if __name__ == "__main__":
    main(sys.argv[1])
