"""CPU: DINO's full-image path and find_fg -- the entry points exist and validate before touching memory, the workspace formula,
the torch port against the fixture written from the real reference, the position-embedding rule against F.interpolate itself,
and the numpy restatement of engines/eval.py:138-144 on hand-built label maps."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dino_full_fixture as fx
import dino_full_port as port
import dino_weights as dw
from nerf_sos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
one, null, big = C.c_void_p(256), None, 1 << 40
NAMES = ("nsos_dino_full_workspace_bytes", "nsos_dino_forward_full", "nsos_dino_interp_pos", "nsos_dino_find_fg_workspace_bytes",
         "nsos_dino_find_fg")
GEOMS = [(756, 1008), (800, 800), (224, 224), (232, 232), (224, 239), (100, 130), (48, 1024), (64, 80)]


def test_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "nerf_sos_hip.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "#define NSOS_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11 == lib.nsos_abi_version()


def expected_ws_bytes(B, h, w):
    """The layout of nsos_dino_full_workspace_bytes: pos T*384, query-0 scores B*6*T, (m, l) B*6*2, x / ln / ao B*T*384 each,
    qkv B*T*1152, the MLP's hidden B*T*1536 (the patch tokens live there first); every section rounded up to 4 floats."""
    T = (h // 16) * (w // 16) + 1
    r4 = lambda n: (n + 3) // 4 * 4   # noqa: E731
    return 4 * (r4(T * 384) + r4(B * 6 * T) + r4(B * 12) + 3 * r4(B * T * 384) + r4(B * T * 1152) + r4(B * T * 1536))


@pytest.mark.parametrize("B,h,w", [(1, 756, 1008), (1, 800, 800), (2, 64, 80), (3, 17, 31), (1, 2048, 2048), (8, 224, 224),
                                   (5, 16, 16 * 16384)])
def test_workspace_formula(B, h, w):
    got = _lib.lib().nsos_dino_full_workspace_bytes(B, h, w)
    assert got == expected_ws_bytes(B, h, w) and got % 16 == 0


def test_workspace_refusals():
    lib = _lib.lib()
    assert lib.nsos_dino_full_workspace_bytes(0, 224, 224) == 0 and lib.nsos_dino_full_workspace_bytes(-1, 224, 224) == 0
    assert lib.nsos_dino_full_workspace_bytes(1025, 224, 224) == 0                   # NSOS_DINO_MAX_BATCH
    assert lib.nsos_dino_full_workspace_bytes(1, 15, 224) == 0 and lib.nsos_dino_full_workspace_bytes(1, 224, 15) == 0   # no patch
    assert lib.nsos_dino_full_workspace_bytes(1, 2048, 2064) == 0                     # 128 x 129 > 16384 tokens
    assert lib.nsos_dino_full_workspace_bytes(1, 2047, 2063) > 0                      # 127 x 128: the remainder is dropped
    assert lib.nsos_dino_full_workspace_bytes(1, 1 << 30, 1 << 30) == 0               # rows * cols far past the cap (no int overflow)
    assert lib.nsos_dino_full_workspace_bytes(300, 2048, 2048) == 0                   # batch * T past the GEMMs' grid
    assert lib.nsos_dino_full_workspace_bytes(255, 2048, 2048) > 0


def _fwd(x=one, B=1, h=64, w=80, flags=0, packed=one, ws=one, nb=big, feat=one):
    return _lib.lib().nsos_dino_forward_full(x, B, h, w, flags, packed, ws, nb, feat, null, null, null, null)


def test_forward_full_rejects_before_launch():
    assert _fwd(x=null) == -1 and _fwd(packed=null) == -1 and _fwd(ws=null) == -1
    assert _fwd(B=0) == -2 and _fwd(B=-2) == -2 and _fwd(h=15) == -2 and _fwd(w=0) == -2 and _fwd(h=-16) == -2
    assert _fwd(flags=4) == -3 and _fwd(flags=8) == -3 and _fwd(flags=-1) == -3
    assert _fwd(h=2048, w=2064) == -3 and _fwd(B=1025) == -3 and _fwd(B=300, h=2048, w=2048) == -3
    assert _fwd(packed=C.c_void_p(260)) == -5 and _fwd(ws=C.c_void_p(264)) == -5 and _fwd(x=C.c_void_p(258)) == -5
    n = _lib.lib().nsos_dino_full_workspace_bytes(2, 64, 80)
    assert _fwd(B=2, nb=n - 4) == -4 and _fwd(nb=0) == -4 and _fwd(B=3, nb=n) == -4


def _fg(labels=one, attn=one, h=64, w=80, out=one, up=null, means=null, flipped=null, ws=one, nb=big):
    return _lib.lib().nsos_dino_find_fg(labels, attn, h, w, out, up, means, flipped, ws, nb, null)


def test_find_fg_rejects_before_launch():
    assert _fg(labels=null) == -1 and _fg(attn=null) == -1 and _fg(out=null) == -1 and _fg(ws=null) == -1
    assert _fg(h=15) == -2 and _fg(w=-3) == -2
    assert _fg(h=2048, w=2064) == -3
    assert _fg(labels=C.c_void_p(258)) == -5 and _fg(means=C.c_void_p(260)) == -5 and _fg(ws=C.c_void_p(264)) == -5
    assert _fg(up=C.c_void_p(257)) == -5 and _fg(flipped=C.c_void_p(258)) == -5
    assert _fg(nb=_lib.lib().nsos_dino_find_fg_workspace_bytes() - 1) == -4


def test_cpu_tensors_raise():
    import nerf_sos_amd
    from nerf_sos_amd import metrics, ops
    m = nerf_sos_amd.DinoViT()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.get_vit_attn_feat_noresize(torch.zeros(1, 3, 64, 80))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_forward_full(torch.zeros(1, 3, 64, 80), torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_find_fg(torch.zeros(64, 80, 1, dtype=torch.int32), torch.zeros(20), 64, 80)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.find_fg(torch.zeros(64, 80, 1, dtype=torch.int32), torch.zeros(64, 80, 3), m)
    with pytest.raises(ValueError, match="outside"):
        ops.dino_full_workspace_floats(1, 2048, 2064)


@pytest.mark.parametrize("h,w", GEOMS + [(16, 16 * 196), (17, 33), (2048, 2048)])
def test_position_rule_is_f_interpolate(h, w):
    """The kernel's rule (nsos_dino_interp_pos: the same host/device function the kernel calls, in fp64, rounded once) against
    models/vision_transformer.py:174-194 run in fp64 on F.interpolate itself: within one fp32 rounding (2^-24 of the value; bar
    2^-23 of the table's max |value|), and the short cut exactly where the reference takes it."""
    from nerf_sos_amd import ops
    pe = dw.make_state("wide", 11)["pos_embed"]
    want = port.interpolate_pos(pe.double(), h, w)[0]
    got = ops.dino_interp_pos(pe, h, w)
    assert got.shape == want.shape
    err = float((got.double() - want).abs().max())
    print(f"{h}x{w}: |rule - F.interpolate fp64| {err:.3e}, scale {float(want.abs().max()):.3e}")
    assert err <= 2.0 ** -23 * float(want.abs().max())
    rows, cols = h // 16, w // 16
    if rows * cols == 196 and h == w:
        assert torch.equal(got, pe[0])
    assert torch.equal(got[0], pe[0, 0])


@pytest.mark.parametrize("h,w", [(756, 1008), (224, 239), (48, 1024)])
def test_numpy_bicubic_restatement(h, w):
    """The documented rule (ATen's coordinate map with 1 / scale_factor, A = -0.75, clamped taps) restated in numpy, against
    F.interpolate in fp64: equal to fp64 rounding."""
    pe = dw.make_state("init", 12)["pos_embed"].double()
    want = port.interpolate_pos(pe, h, w)[0, 1:].numpy()
    got = port.bicubic_rule(pe[0, 1:].reshape(14, 14, 384).numpy(), h // 16, w // 16).reshape(-1, 384)
    assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max())
    # ATen's map uses 1 / scale_factor, not in / out: the two differ here
    assert abs(1.0 / ((h // 16 + 0.1) / 14.0) - 14.0 / (h // 16)) > 0 or abs(1.0 / ((w // 16 + 0.1) / 14.0) - 14.0 / (w // 16)) > 0


@pytest.mark.parametrize("ci", range(9))
def test_port_reproduces_the_reference(ci):
    """The port (with interpolation) on regenerated weights and inputs gives the reference's fp32 outputs (bit for bit where the
    BLAS / thread count matches the generator's; never further than the GPU's bar)."""
    assert fx.n_cases() == 9
    c = fx.case(ci)
    sd = dw.make_state(c["kind"], fx.meta()["seeds"][c["kind"]])
    x = torch.from_numpy(c["input"])
    out = port.get_vit_attn_feat_noresize(sd, port.eval_dino_in(x))
    out["feat"] = out["feat"][:, ::c["feat_stride"]]
    for k in fx.OUTPUTS:
        got, want = out[k].numpy(), c["ref32"][k]
        assert got.shape == want.shape
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert err <= fx.bar(c, k), (k, err, fx.bar(c, k))
    assert out["attn"].shape == (c["B"], 1, c["rows"] * c["cols"])
    for k in ("attn", "cls_"):
        assert float(np.abs(c["ref32"][k].astype(np.float64) - c["ref64"][k]).max()) <= c["e32"][k]
        assert 4 * c["e32"][k] <= 1e-4 * c["scale"][k]


def _disc(h, w, cy, cx, r):
    y, x = np.mgrid[0:h, 0:w]
    return ((y - cy) ** 2 + (x - cx) ** 2) <= r * r


def test_find_fg_restatement_on_hand_built_maps():
    """engines/eval.py:142-144 restated (dino_full_port.find_fg_numpy) on maps whose answer is known by construction."""
    h, w = 64, 80
    bright = _disc(h, w, 30, 40, 15)
    attn = np.where(bright, 0.9, 0.1).astype(np.float32)[..., None]
    # disc: the attended disc labelled 0 -> flipped to 1
    lab = np.where(bright, 0, 1).astype(np.int32)[..., None]
    out, flip = port.find_fg_numpy(attn, lab)
    assert flip and np.array_equal(out, 1 - lab)
    out, flip = port.find_fg_numpy(attn, 1 - lab)     # already oriented
    assert not flip and np.array_equal(out, 1 - lab)
    # halves: left half brighter on average
    ramp = np.linspace(1.0, 0.0, w, dtype=np.float32)[None, :, None].repeat(h, 0)
    halves = (np.arange(w)[None, :, None] >= w // 2).astype(np.int32).repeat(h, 0)   # right half = 1: darker -> flip
    out, flip = port.find_fg_numpy(ramp, halves)
    assert flip and np.array_equal(out, 1 - halves)
    # an empty cluster: the mean of nothing is NaN, the comparison False, nothing flips
    for only in (0, 1):
        lab = np.full((h, w, 1), only, np.int32)
        out, flip = port.find_fg_numpy(attn, lab)
        assert not flip and np.array_equal(out, lab)
    # three clusters: 2 takes part in neither mean but is mapped by 1 - label (2 -> -1)
    lab = np.where(bright, 0, 1).astype(np.int32)[..., None]
    lab[:8] = 2
    out, flip = port.find_fg_numpy(attn, lab)
    assert flip and np.array_equal(out, 1 - lab) and (out[:8] == -1).all()
    m0, m1 = attn[lab == 0].mean(), attn[lab == 1].mean()
    assert m1 < m0


def test_upsample_is_aten_size_rule():
    """eval.py:140's F.interpolate(attn, (H, W)) is the size= nearest rule min(floor(dst * (float)rows / H), rows - 1), which is not
    dst // 16 when H is not a multiple of 16 (756 = 47 * 16 + 4)."""
    rows, cols, h, w = 47, 63, 756, 1008
    a = torch.arange(rows * cols, dtype=torch.float32).reshape(1, 1, rows * cols)
    up = port.upsample_attn(a, h, w)[..., 0].numpy().astype(np.int64)
    sy = np.minimum(np.floor(np.arange(h, dtype=np.float32) * (np.float32(rows) / np.float32(h))), rows - 1).astype(np.int64)
    sx = np.minimum(np.floor(np.arange(w, dtype=np.float32) * (np.float32(cols) / np.float32(w))), cols - 1).astype(np.int64)
    assert np.array_equal(up, sy[:, None] * cols + sx[None, :])
    assert not np.array_equal(sy, np.arange(h) // 16)
    assert math.floor(755 * (47 / 756)) == 46
