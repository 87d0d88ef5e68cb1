"""Loader of the full-image DINO fixtures written by tests/golden/make_goldens_dino_full.py (a plain helper, not a conftest).
The inputs are regenerated from their seeds and checked against the sha256 the generator recorded."""
import hashlib
import json
import os

import numpy as np

import dino_fixture

GOLDEN = dino_fixture.GOLDEN
OUTPUTS = ("attn", "cls_", "feat")
bar = dino_fixture.bar          # max(4 * e32, 1e-6 * scale), capped at 1e-4 * scale
_cache = {}


def _npz(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _cache[name]


def meta():
    if "meta" not in _cache:
        _cache["meta"] = json.loads(str(_npz("dino_full")["meta"]))
    return _cache["meta"]


def n_cases():
    return len(meta()["cases"])


def make_input(c):
    """rgb [B,H,W,3] float32 as rendered (the generator's default_rng(seed).random draw)."""
    x = np.random.default_rng(c["seed"]).random((c["B"], c["h"], c["w"], 3), dtype=np.float32)
    assert hashlib.sha256(np.ascontiguousarray(x, dtype="<f4").tobytes()).hexdigest() == c["input_sha256"], "input differs from the generator's"
    return x


def case(ci):
    """Case ci: the table entry plus input, fp32 / fp64 outputs (feat: rows 0, s, 2s, .. with s = feat_stride; fp64 of image 0),
    e32 / scale per output."""
    c = dict(meta()["cases"][ci])
    d = _npz(f"dino_full_c{ci}")
    c.update(input=make_input(c), e32=dict(zip(OUTPUTS, d["e32"].tolist())), scale=dict(zip(OUTPUTS, d["scale"].tolist())),
             ref32={"attn": d["attn32"], "cls_": d["cls32"], "feat": _npz(f"dino_full_feat32_c{ci}")["feat"]},
             ref64={"attn": d["attn64"], "cls_": d["cls64"], "feat0": _npz(f"dino_full_feat64_c{ci}")["feat"]})
    return c
