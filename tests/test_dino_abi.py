"""CPU: the DINO ViT-S/16 entry points exist, validate before touching memory, DinoViT carries the checkpoint's keys and shapes,
the weight formula and the torch port reproduce the fixture (which was written from the real reference), and nothing runs on a
CPU tensor."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dino_fixture as fx
import dino_port as port
import dino_weights as dw
from helpers import state_sha
from nerf_sos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
one, null, big = C.c_void_p(256), None, 1 << 40
NAMES = ("nsos_dino_packed_bytes", "nsos_dino_pack", "nsos_dino_workspace_bytes", "nsos_dino_forward", "nsos_dino_resize_indices")


def test_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "nerf_sos_hip.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "#define NSOS_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11 == lib.nsos_abi_version()


def test_sizes():
    lib = _lib.lib()
    n_params = sum(int(np.prod(s)) for k, s in dw.key_shapes() if not k.startswith("norm.") and k != "cls_token")
    assert lib.nsos_dino_packed_bytes() == 4 * n_params           # cls_token is folded into row 0 of pos_embed, norm.* dropped
    w1, w8 = lib.nsos_dino_workspace_bytes(1), lib.nsos_dino_workspace_bytes(8)
    assert w1 > 0 and w8 == 8 * w1 and w1 % 16 == 0 and lib.nsos_dino_workspace_bytes(64) == 64 * w1
    assert lib.nsos_dino_workspace_bytes(0) == 0 and lib.nsos_dino_workspace_bytes(-3) == 0 and lib.nsos_dino_workspace_bytes(1 << 20) == 0


def _fwd(x=one, B=2, h=64, w=64, stride=6, flags=3, packed=one, ws=one, nb=big, feat=one):
    return _lib.lib().nsos_dino_forward(x, B, h, w, stride, flags, packed, ws, nb, feat, null, null, null, null, null)


def test_forward_rejects_before_launch():
    assert _fwd(x=null) == -1 and _fwd(packed=null) == -1 and _fwd(ws=null) == -1
    assert _fwd(B=0) == -2 and _fwd(B=-4) == -2 and _fwd(h=0) == -2 and _fwd(w=-1) == -2
    assert _fwd(stride=0) == -2 and _fwd(stride=-2) == -2            # P * stride of 0: no intermediate image
    assert _fwd(flags=8) == -3 and _fwd(flags=4 | 1) == -3 and _fwd(flags=4 | 2) == -3
    assert _fwd(flags=4, h=64, w=64) == -2                           # a prepared input is 224 x 224
    assert _fwd(B=(1 << 20)) == -3 and _fwd(h=1 << 20) == -3 and _fwd(stride=1 << 20) == -3
    assert _fwd(packed=C.c_void_p(260)) == -5 and _fwd(ws=C.c_void_p(264)) == -5 and _fwd(x=C.c_void_p(258)) == -5
    assert _fwd(nb=_lib.lib().nsos_dino_workspace_bytes(2) - 4) == -4 and _fwd(nb=0) == -4
    assert _fwd(B=3, nb=_lib.lib().nsos_dino_workspace_bytes(2)) == -4


def test_pack_rejects_before_launch():
    lib = _lib.lib()
    ts = _lib.DinoTensors()
    n = lib.nsos_dino_packed_bytes()
    assert lib.nsos_dino_pack(null, one, n, null) == -1
    assert lib.nsos_dino_pack(C.byref(ts), one, n, null) == -1       # every tensor pointer is NULL
    for f, _ in ts._fields_[:4]:
        setattr(ts, f, 256)
    for b in ts.blocks:
        for f, _ in b._fields_:
            setattr(b, f, 256)
    assert lib.nsos_dino_pack(C.byref(ts), null, n, null) == -1
    assert lib.nsos_dino_pack(C.byref(ts), C.c_void_p(260), n, null) == -5
    assert lib.nsos_dino_pack(C.byref(ts), one, n - 4, null) == -4
    ts.blocks[7].fc2_b = None
    assert lib.nsos_dino_pack(C.byref(ts), one, n, null) == -1


@pytest.mark.parametrize("size,stride", [(64, 6), (32, 1), (48, 5), (224, 0), (40, 0), (56, 0), (64, 1), (17, 3), (100, 7), (300, 0), (7, 13)])
def test_resize_indices_are_torch_nearest(size, stride):
    """The host twin of the prepare kernel's index rule against F.interpolate (nearest) itself, both resizes composed."""
    from nerf_sos_amd import ops
    ramp = torch.arange(size, dtype=torch.float32).reshape(1, 1, size, 1).expand(1, 1, size, 2)
    x = ramp
    if stride:
        x = torch.nn.functional.interpolate(x, (size * stride, 2))
    x = torch.nn.functional.interpolate(x, size=(224, 2))
    assert ops.dino_resize_indices(size, stride) == x[0, 0, :, 0].to(torch.int64).tolist()
    lib = _lib.lib()
    assert lib.nsos_dino_resize_indices(size, stride, None) == -1 and lib.nsos_dino_resize_indices(0, 1, (C.c_int32 * 224)()) == -2


def test_module_has_the_checkpoint_keys_and_shapes():
    import nerf_sos_amd
    m = nerf_sos_amd.DinoViT()
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == fx.meta()["keys"] and len(got) == 150                 # the list the generator read off the real vit_small
    assert got == [[k, list(s)] for k, s in dw.key_shapes()]
    assert not any(p.requires_grad for p in m.parameters())
    m.load_state_dict(dw.make_state("init", 12))                      # strict: a checkpoint file loads as it is


def test_cpu_tensor_raises():
    import nerf_sos_amd
    m = nerf_sos_amd.DinoViT()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.get_vit_attn_feat(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.patch_features(torch.zeros(1, 32, 32, 3), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nerf_sos_amd.ops.dino_forward(torch.zeros(1, 3, 32, 32), torch.zeros(4), 0)


@pytest.mark.parametrize("kind", dw.KINDS)
def test_make_state_is_pinned(kind):
    m = fx.meta()
    assert state_sha(dw.make_state(kind, m["seeds"][kind])) == m["state_sha256"][kind]


@pytest.mark.parametrize("ci", range(6))
def test_port_reproduces_the_reference(ci):
    """The port on regenerated weights gives the reference's fp32 outputs bit for bit (same ATen kernels on a CPU: both the formula
    and the port are pinned), and the fixture's e32 is what separates them from its fp64 outputs."""
    assert fx.n_cases() == 6
    c = fx.case(ci)
    sd = dw.make_state(c["kind"], fx.meta()["seeds"][c["kind"]])
    x = torch.from_numpy(c["input"])
    out = port.patch_features(sd, x, c["stride"]) if c["mode"] == "patch" else port.get_vit_attn_feat(sd, x)
    for k in fx.OUTPUTS:
        got, want = out[k].numpy(), c["ref32"][k]
        assert got.shape == want.shape
        err = float(np.abs(got.astype(np.float64) - want).max())
        # bit-equal where the BLAS / thread count matches the generator's; never further than the bar the GPU path gets
        assert err <= fx.bar(c, k), (k, err, fx.bar(c, k))
    assert float(np.abs(c["ref32"]["feat"][0].astype(np.float64) - c["ref64"]["feat0"]).max()) <= c["e32"]["feat"]
    assert float(np.abs(c["ref32"]["cls_"].astype(np.float64) - c["ref64"]["cls_"]).max()) == c["e32"]["cls_"]
    if ci == 2:
        p = dict(np.load(os.path.join(fx.GOLDEN, "dino_vit_prepared.npz")))
        assert np.array_equal(port.prepare(x, c["stride"])[int(p["index"])].numpy(), p["image"])
