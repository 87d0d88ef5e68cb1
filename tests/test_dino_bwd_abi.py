"""CPU: the entry points of DINO's backward to the input exist and validate before touching memory, the Python interface refuses
what it cannot do with the reason in the message, and the fixture's stored gradient is what the torch port gives in fp64."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dino_bwd_fixture as bfx
import dino_weights as dw
from nerf_sos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
one, null, big = C.c_void_p(256), None, 1 << 40
NAMES = ("nsos_dino_saved_bytes", "nsos_dino_forward_save", "nsos_dino_backward_packed_bytes", "nsos_dino_pack_backward",
         "nsos_dino_backward_workspace_bytes", "nsos_dino_backward")


def test_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "nerf_sos_hip.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "#define NSOS_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11 == lib.nsos_abi_version()
    from nerf_sos_amd import ops
    for n in ("dino_backward", "dino_backward_workspace", "dino_backward_workspace_floats", "dino_pack_backward", "dino_saved_floats"):
        assert callable(getattr(ops, n)), n


def test_sizes():
    lib = _lib.lib()
    for fn in (lib.nsos_dino_backward_workspace_bytes, lib.nsos_dino_saved_bytes):
        w1 = fn(1)
        assert w1 > 0 and w1 % 16 == 0 and fn(8) == 8 * w1 and fn(1024) == 1024 * w1
        assert fn(0) == 0 and fn(-3) == 0 and fn(1025) == 0 and fn(1 << 20) == 0
    assert lib.nsos_dino_saved_bytes(1) == 12 * 197 * 384 * 4
    mats = sum(int(np.prod(s)) for k, s in dw.key_shapes() if k.endswith(("qkv.weight", "proj.weight", "fc1.weight", "fc2.weight")))
    assert lib.nsos_dino_backward_packed_bytes() == 4 * (mats + 1536)      # every matrix once, and the GEMM tile's zero bias


def _bwd(B=2, h=64, w=64, stride=6, flags=3, packed=one, pb=one, saved=one, g_feat=one, g_cls=one, ws=one, nb=big, g_in=one, g_blocks=null):
    return _lib.lib().nsos_dino_backward(B, h, w, stride, flags, packed, pb, saved, g_feat, g_cls, ws, nb, g_in, g_blocks, null)


def test_backward_rejects_before_launch_in_the_documented_order():
    need = _lib.lib().nsos_dino_backward_workspace_bytes
    # NULL pointer
    assert _bwd(packed=null) == -1 and _bwd(pb=null) == -1 and _bwd(saved=null) == -1 and _bwd(ws=null) == -1 and _bwd(g_in=null) == -1
    assert _bwd(g_feat=null, g_cls=null) == -1                          # one upstream gradient may be NULL, not both
    # shape, flag bits, PREPARED, STEP1, size limits: nsos_dino_forward's
    assert _bwd(B=0) == -2 and _bwd(B=-4) == -2 and _bwd(h=0) == -2 and _bwd(w=-1) == -2
    assert _bwd(flags=8) == -3 and _bwd(flags=4 | 1) == -3 and _bwd(flags=4 | 2) == -3
    assert _bwd(flags=4, h=64, w=64) == -2
    assert _bwd(stride=0) == -2 and _bwd(stride=1 << 20) == -3
    assert _bwd(B=(1 << 20)) == -3 and _bwd(h=1 << 20) == -3
    # alignment
    for k in ("packed", "pb", "saved", "ws"):
        assert _bwd(**{k: C.c_void_p(264)}) == -5, k
    for k in ("g_feat", "g_cls", "g_in", "g_blocks"):
        assert _bwd(**{k: C.c_void_p(258)}) == -5, k
    # workspace size
    assert _bwd(nb=need(2) - 4) == -4 and _bwd(nb=0) == -4 and _bwd(B=3, nb=need(2)) == -4
    # a call wrong in two ways reports the first of the order
    assert _bwd(saved=null, B=0) == -1 and _bwd(B=0, flags=8) == -2 and _bwd(flags=8, ws=C.c_void_p(264)) == -3
    assert _bwd(ws=C.c_void_p(264), nb=0) == -5


def test_forward_save_and_pack_backward_reject_before_launch():
    lib = _lib.lib()

    def save(x=one, B=2, flags=3, packed=one, ws=one, nb=big, saved=one):
        return lib.nsos_dino_forward_save(x, B, 64, 64, 6, flags, packed, ws, nb, one, null, null, saved, null)
    assert save(saved=null) == -1 and save(x=null) == -1 and save(B=0) == -2 and save(flags=8) == -3
    assert save(saved=C.c_void_p(264)) == -5 and save(nb=lib.nsos_dino_workspace_bytes(2) - 4) == -4
    ts = _lib.DinoTensors()
    n = lib.nsos_dino_backward_packed_bytes()
    assert lib.nsos_dino_pack_backward(null, one, n, null) == -1 and lib.nsos_dino_pack_backward(C.byref(ts), one, n, null) == -1
    for f, _ in ts._fields_[:4]:
        setattr(ts, f, 256)
    for b in ts.blocks:
        for f, _ in b._fields_:
            setattr(b, f, 256)
    assert lib.nsos_dino_pack_backward(C.byref(ts), null, n, null) == -1
    assert lib.nsos_dino_pack_backward(C.byref(ts), C.c_void_p(260), n, null) == -5
    assert lib.nsos_dino_pack_backward(C.byref(ts), one, n - 4, null) == -4


def test_module_refuses_with_the_reason():
    import nerf_sos_amd
    m = nerf_sos_amd.DinoViT()
    rgb = torch.zeros(1, 32, 32, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.patch_features(rgb, 2, differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.get_vit_attn_feat(torch.zeros(1, 3, 32, 32, requires_grad=True), differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nerf_sos_amd.ops.dino_backward((1, 32, 32, 3), 3, 2, torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(1, 196, 384), None)
    out = {"feat": torch.zeros(1, 196, 384), "cls_": torch.zeros(1, 384)}
    with pytest.raises(ValueError, match="out="):
        m.patch_features(rgb, 2, differentiable=True, out=out)
    with pytest.raises(ValueError, match="full-image"):
        m.get_vit_attn_feat_noresize(torch.zeros(1, 3, 32, 32), differentiable=True)
    m16 = nerf_sos_amd.DinoViT("bf16")
    with pytest.raises(ValueError, match="fp32"):
        m16.patch_features(rgb, 2, differentiable=True)
    with pytest.raises(ValueError, match="fp32"):
        m16.prepare(1, backward=True)
    with pytest.raises(ValueError, match="g_feat or g_cls"):
        nerf_sos_amd.ops.dino_backward((1, 32, 32, 3), 3, 2, None, None, None, None, None)


def test_step_refuses_dino_grad_without_an_extractor():
    import nerf_sos_amd
    from nerf_sos_amd import sharding
    rays = torch.zeros(2, 1, 16, 16, 3)
    feat, cls_ = torch.zeros(1, 384, 14, 14), torch.zeros(1, 384)
    with pytest.raises(ValueError, match="dino_grad"):
        sharding.sharded_patch_step(None, rays, (2.0, 6.0), 1, feat, cls_, dino_grad=True)
    out = {"feat": torch.zeros(1, 196, 384), "cls_": torch.zeros(1, 384)}
    with pytest.raises(ValueError, match="dino_grad"):
        sharding.sharded_patch_step(None, rays, (2.0, 6.0), 1, None, None, dino=nerf_sos_amd.DinoViT(), patch_stride=2, dino_out=out,
                                    dino_grad=True)


def test_fixture_shape_and_the_port_reproduces_the_stored_gradient():
    """The generator asserted the port's fp64 gradient equal to the reference module's; here the port, in fp64 on this CPU, against
    what the generator stored (case 3: one 40 x 56 image)."""
    m = bfx.meta()
    assert len(m["cases"]) == len(bfx.CASES) == 6
    for ci in range(6):
        c = bfx.case(ci)
        assert c["g64"].shape == c["input"].shape and c["g64"].dtype == np.float64
        assert 0 < 4 * c["e32"] <= 1e-4 * c["scale"] and c["scale"] == float(np.abs(c["g64"]).max())
    c = bfx.case(3)
    got = bfx.port_input_grad(dw.make_state(c["kind"], m["seeds"][c["kind"]]), c, torch.float64).numpy()
    err = float(np.abs(got - c["g64"]).max())
    print(f"case 3: |port fp64 - stored fp64| {err:.3e}, scale {c['scale']:.3e}")
    assert err <= 1e-10 * c["scale"]
    c4 = bfx.case(4)                                                  # pixels no pixel of the 224 x 224 image reads: exact zeros
    from nerf_sos_amd import ops
    rows, cols = set(ops.dino_resize_indices(250)), set(ops.dino_resize_indices(230))
    unmapped = ~(np.isin(np.arange(250), list(rows))[:, None] & np.isin(np.arange(230), list(cols))[None, :])
    assert unmapped.sum() > 0 and (c4["g64"][0][:, unmapped] == 0.0).all() and (c4["g64"][0][:, ~unmapped] != 0.0).all()
    blocks = bfx.block_grads()
    assert sorted(blocks) == [0, 5, 11] and all(g.shape == (bfx.BLOCK_ROWS, 384) for g, _, _ in blocks.values())
