"""Writes tests/golden/dino_vit16.npz, the yardstick of the 16-bit DINO path:  python tests/golden/make_goldens_dino16.py

Needs no reference checkout: it reads only committed fixtures (dino_vit_c*.npz, dino_vit_feat64_c*.npz, dino_vit_block{0,5}.npz:
the fp64 outputs of the real reference) and tests/dino_weights.py (sha256 of every generated state checked against the fixture's),
and runs tests/dino16_model.py -- the torch port with the operands of every matrix product rounded to 16 bits -- on the CPU.
Numbers only (a few KB):

  e16         [case 0..5][fp16, bf16][placement A, B][attn, cls_, feat]  max |model - fp64| (feat: image 0, the one with an fp64 fixture)
  dsim        [case][precision][placement]   max |sim(model cls_) - sim(fp64 cls_)| of the cosine-similarity matrix (NaN for B = 1)
  min_cos     [case][precision][placement]   smallest cosine of a model feat row to its fp64 row (image 0)
  block_e16   [block 0, 5][precision][placement]  max |model block output - fp64| on tokens 0..49 of image 0 of case 0
  max_operand [init, wide, peaky][precision]      the largest |operand| of any matrix product (fp16 rounds beyond 65504 to infinity)
  meta        JSON: the axis labels above

It prints, per precision, the range over the six cases of e16 / scale for placement A; these reproduce the table of DESIGN.md
4.10.2 ("CPU model") to its printed digits, and the ratio of placement B to A.  Asserted here: no non-finite value anywhere, the
model's negatives equal the fixture's argmin in every multi-image case, and the negatives test keeps its cases: gap > 4 * dsim (both
placements) holds for at least two of the three multi-image cases in fp16 and at least one in bf16.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dino16_model as m16        # noqa: E402
import dino_fixture as fx         # noqa: E402
import dino_port as port          # noqa: E402
import dino_weights as dw         # noqa: E402
from helpers import state_sha     # noqa: E402

PRECISIONS = ("fp16", "bf16")
BLOCKS = (0, 5)


def worst(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def sim64(cls_):
    c = torch.from_numpy(np.asarray(cls_, np.float64))
    return F.cosine_similarity(c.unsqueeze(0), c.unsqueeze(1), dim=2)


def main():
    torch.set_num_threads(8)
    n = fx.n_cases()
    e16 = np.zeros((n, 2, 2, 3))
    dsim = np.full((n, 2, 2), np.nan)
    min_cos = np.zeros((n, 2, 2))
    block_e16 = np.zeros((len(BLOCKS), 2, 2))
    max_operand = np.zeros((len(dw.KINDS), 2))
    states = {}
    for kind in dw.KINDS:
        states[kind] = dw.make_state(kind, fx.meta()["seeds"][kind])
        assert state_sha(states[kind]) == fx.meta()["state_sha256"][kind], kind
    for ci in range(n):
        c = fx.case(ci)
        x = torch.from_numpy(c["input"])
        for pi, prec in enumerate(PRECISIONS):
            for li, plc in enumerate(m16.PLACEMENTS):
                stats = {}
                o = m16.run_case(states[c["kind"]], c, x, prec, plc, want_blocks=(ci == 0), stats=stats)
                ki = dw.KINDS.index(c["kind"])
                max_operand[ki, pi] = max(max_operand[ki, pi], stats["max_operand"])
                for oi, k in enumerate(fx.OUTPUTS):
                    got = o[k].numpy()
                    assert np.isfinite(got).all(), (ci, prec, plc, k)
                    e16[ci, pi, li, oi] = worst(got[0], c["ref64"]["feat0"]) if k == "feat" else worst(got, c["ref64"][k])
                r64 = torch.from_numpy(np.asarray(c["ref64"]["feat0"], np.float64))
                min_cos[ci, pi, li] = F.cosine_similarity(o["feat"][0].double(), r64, dim=1).min().item()
                if c["B"] > 1:
                    dsim[ci, pi, li] = float((sim64(o["cls_"].numpy()) - sim64(c["ref64"]["cls_"])).abs().max())
                    _, am = port.similarity_argmin(o["cls_"])
                    assert am.tolist() == c["argmin"].tolist(), (ci, prec, plc)
                if ci == 0:
                    for bi, k in enumerate(BLOCKS):
                        d = dict(np.load(os.path.join(fx.GOLDEN, f"dino_vit_block{k}.npz")))
                        block_e16[bi, pi, li] = worst(o["blocks"][k][0, :d["out64"].shape[0]].numpy(), d["out64"])
                print(f"case {ci} {c['kind']:5s} B{c['B']} {prec} {plc}: " +
                      " ".join(f"{k} {e16[ci, pi, li, oi] / c['scale'][k]:.2e}" for oi, k in enumerate(fx.OUTPUTS)) +
                      f" min cos {min_cos[ci, pi, li]:.6f} dsim {dsim[ci, pi, li]:.2e} gap {c['gap']:.2e}", flush=True)
    scale = np.array([[fx.case(ci)["scale"][k] for k in fx.OUTPUTS] for ci in range(n)])
    for pi, prec in enumerate(PRECISIONS):
        rel = e16[:, pi, 0, :] / scale
        print(f"{prec} placement A, e16 / scale over the cases: " +
              ", ".join(f"{k} {rel[:, oi].min():.1e} .. {rel[:, oi].max():.1e}" for oi, k in enumerate(fx.OUTPUTS)) +
              f"; min cosine {min_cos[:, pi, 0].min():.6f}")
        ratio = e16[:, pi, 1, :] / e16[:, pi, 0, :]
        print(f"{prec} placement B / A: {ratio.min():.2f} .. {ratio.max():.2f}")
        multi = [ci for ci in range(n) if fx.case(ci)["B"] > 1]
        ok = [ci for ci in multi if fx.case(ci)["gap"] > 4.0 * np.nanmax(dsim[ci, pi])]
        print(f"{prec} negatives cases with gap > 4 * dsim: {ok} of {multi}")
        assert len(ok) >= (2 if prec == "fp16" else 1), (prec, ok)
    for ki, kind in enumerate(dw.KINDS):
        print(f"largest |operand|, {kind}: fp16 {max_operand[ki, 0]:.1f}, bf16 {max_operand[ki, 1]:.1f}")
    assert max_operand.max() < 65504.0 / 16, "an operand within a factor 16 of fp16's largest finite value"
    meta = dict(precisions=PRECISIONS, placements=m16.PLACEMENTS, outputs=fx.OUTPUTS, kinds=dw.KINDS, blocks=BLOCKS)
    np.savez(os.path.join(HERE, "dino_vit16.npz"), e16=e16, dsim=dsim, min_cos=min_cos, block_e16=block_e16, max_operand=max_operand,
             meta=np.array(json.dumps(meta)))
    print("wrote dino_vit16.npz")


if __name__ == "__main__":
    main()
