"""Loader of the DINO fixtures written by tests/golden/make_goldens_dino.py (a plain helper, not a conftest)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTPUTS = ("attn", "cls_", "feat")
_cache = {}


def _npz(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _cache[name]


def meta():
    if "meta" not in _cache:
        _cache["meta"] = json.loads(str(_npz("dino_vit")["meta"]))
    return _cache["meta"]


def feat32(image):
    """The reference's fp32 feat [196,384] of global image number `image`."""
    chunk = meta()["chunk"]
    return _npz(f"dino_vit_feat32_{image // chunk}")["feat"][image % chunk]


def case(ci):
    """Case ci: the table entry plus input, fp32 / fp64 outputs, e32 / scale per output."""
    c = dict(meta()["cases"][ci])
    d = _npz(f"dino_vit_c{ci}")
    c.update(input=d["input"], argmin=d["argmin"], gap=float(d["gap"]),
             e32=dict(zip(OUTPUTS, d["e32"].tolist())), scale=dict(zip(OUTPUTS, d["scale"].tolist())),
             ref32={"attn": d["attn32"], "cls_": d["cls32"],
                    "feat": np.stack([feat32(c["first_image"] + b) for b in range(c["B"])])},
             ref64={"attn": d["attn64"], "cls_": d["cls64"], "feat0": _npz(f"dino_vit_feat64_c{ci}")["feat"]})
    return c


def n_cases():
    return len(meta()["cases"])


def bar(c, k):
    """The project's fp32 bar against fp64 (tests/test_gpu_losses_edges.py): max(4 * e32, 1e-6 * scale), and never above the
    end-to-end bar of 1e-4 * scale (the generator asserts 4 * e32 <= 1e-4 * scale, so the cap only ever confirms it)."""
    return min(max(4.0 * c["e32"][k], 1e-6 * c["scale"][k]), 1e-4 * c["scale"][k])
