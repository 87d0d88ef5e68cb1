"""CPU: the 16-bit DINO entry points exist and validate before touching memory, DinoViT.precision is checked on assignment, the
full-image path refuses a 16-bit precision, the built 16-bit kernels use no scratch, and tests/dino16_model.py reproduces the
committed yardstick (tests/golden/dino_vit16.npz) on a small case."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import dino16_model as m16
import dino_fixture as fx
import dino_weights as dw
from nerf_sos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
one, null, big = C.c_void_p(256), None, 1 << 40
NAMES = ("nsos_dino_packed16_bytes", "nsos_dino_pack16", "nsos_dino_workspace16_bytes", "nsos_dino_forward16")
F16, BF16 = 1, 2          # NSOS_DTYPE_F16 / NSOS_DTYPE_BF16


def golden16():
    d = dict(np.load(os.path.join(fx.GOLDEN, "dino_vit16.npz")))
    d["meta"] = json.loads(str(d["meta"]))
    return d


def test_symbols_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "nerf_sos_hip.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert "#define NSOS_ABI_VERSION 11" in header and _lib.ABI_VERSION == 11 == lib.nsos_abi_version()
    assert re.search(r"NSOS_DTYPE_F32 = 0, NSOS_DTYPE_F16 = 1, NSOS_DTYPE_BF16 = 2", header)


def test_sizes():
    lib = _lib.lib()
    shapes = [(k, s) for k, s in dw.key_shapes() if not k.startswith("norm.") and k != "cls_token"]
    n_matrix = sum(int(np.prod(s)) for k, s in shapes if len(s) in (2, 4))      # nn.Linear weights and the patch convolution
    n_fp32 = sum(int(np.prod(s)) for k, s in shapes if len(s) not in (2, 4))    # pos_embed (cls_token folded in), biases, LayerNorm
    assert n_matrix == 768 * 384 + 12 * (3 * 384 * 384 + 384 * 384 + 2 * 384 * 1536)
    assert lib.nsos_dino_packed16_bytes() == 4 * n_fp32 + 2 * n_matrix
    assert lib.nsos_dino_packed16_bytes() % 16 == 0 and lib.nsos_dino_packed16_bytes() < lib.nsos_dino_packed_bytes() * 0.51
    # per image: fp32 x [197,384] and softmax row 0 [6,196]; 16-bit LayerNorm output, qkv, attention output, hidden, im2col tokens
    per_image = 4 * (197 * 384 + 6 * 196) + 2 * (197 * 384 * 2 + 197 * 1152 + 197 * 1536 + 196 * 768)
    w1 = lib.nsos_dino_workspace16_bytes(1)
    assert w1 == per_image and w1 % 16 == 0
    assert lib.nsos_dino_workspace16_bytes(8) == 8 * w1 and lib.nsos_dino_workspace16_bytes(1024) == 1024 * w1
    assert lib.nsos_dino_workspace16_bytes(0) == 0 and lib.nsos_dino_workspace16_bytes(-3) == 0 and lib.nsos_dino_workspace16_bytes(1 << 20) == 0


def _fwd(x=one, B=2, h=64, w=64, stride=6, flags=3, prec=F16, packed=one, ws=one, nb=big, feat=one):
    return _lib.lib().nsos_dino_forward16(x, B, h, w, stride, flags, prec, packed, ws, nb, feat, null, null, null, null, null)


def test_forward16_rejects_before_launch():
    lib = _lib.lib()
    assert _fwd(prec=0) == -3 and _fwd(prec=3) == -3 and _fwd(prec=-1) == -3 and _fwd(prec=7) == -3     # fp32 is nsos_dino_forward
    for prec in (F16, BF16):
        assert _fwd(prec=prec, x=null) == -1 and _fwd(prec=prec, packed=null) == -1 and _fwd(prec=prec, ws=null) == -1
        assert _fwd(prec=prec, B=0) == -2 and _fwd(prec=prec, B=-4) == -2 and _fwd(prec=prec, h=0) == -2 and _fwd(prec=prec, w=-1) == -2
        assert _fwd(prec=prec, stride=0) == -2 and _fwd(prec=prec, stride=-2) == -2
        assert _fwd(prec=prec, flags=8) == -3 and _fwd(prec=prec, flags=4 | 1) == -3 and _fwd(prec=prec, flags=4 | 2) == -3
        assert _fwd(prec=prec, flags=4, h=64, w=64) == -2
        assert _fwd(prec=prec, B=(1 << 20)) == -3 and _fwd(prec=prec, h=1 << 20) == -3 and _fwd(prec=prec, stride=1 << 20) == -3
        assert _fwd(prec=prec, packed=C.c_void_p(260)) == -5 and _fwd(prec=prec, ws=C.c_void_p(264)) == -5
        assert _fwd(prec=prec, x=C.c_void_p(258)) == -5
        assert _fwd(prec=prec, nb=lib.nsos_dino_workspace16_bytes(2) - 4) == -4 and _fwd(prec=prec, nb=0) == -4
        assert _fwd(prec=prec, B=3, nb=lib.nsos_dino_workspace16_bytes(2)) == -4


def test_pack16_rejects_before_launch():
    lib = _lib.lib()
    ts = _lib.DinoTensors()
    n = lib.nsos_dino_packed16_bytes()
    assert lib.nsos_dino_pack16(null, F16, one, n, null) == -1
    assert lib.nsos_dino_pack16(C.byref(ts), F16, one, n, null) == -1       # every tensor pointer is NULL
    for f, _ in ts._fields_[:4]:
        setattr(ts, f, 256)
    for b in ts.blocks:
        for f, _ in b._fields_:
            setattr(b, f, 256)
    for prec in (F16, BF16):
        assert lib.nsos_dino_pack16(C.byref(ts), prec, null, n, null) == -1
        assert lib.nsos_dino_pack16(C.byref(ts), prec, C.c_void_p(260), n, null) == -5
        assert lib.nsos_dino_pack16(C.byref(ts), prec, one, n - 2, null) == -4
    assert lib.nsos_dino_pack16(C.byref(ts), 0, one, n, null) == -3 and lib.nsos_dino_pack16(C.byref(ts), 3, one, n, null) == -3
    ts.blocks[7].fc2_b = None
    assert lib.nsos_dino_pack16(C.byref(ts), BF16, one, n, null) == -1


def test_precision_attribute_is_validated():
    import nerf_sos_amd
    m = nerf_sos_amd.DinoViT()
    assert m.precision == "fp32"
    for p in ("fp16", "bf16", "fp32"):
        m.precision = p
        assert m.precision == p
        assert nerf_sos_amd.DinoViT(precision=p).precision == p
    for bad in ("fp8", "fp16x3", "", None, 16, "FP16"):
        with pytest.raises(ValueError, match="precision"):
            m.precision = bad
        assert m.precision == "fp32"
    with pytest.raises(ValueError, match="precision"):
        nerf_sos_amd.DinoViT(precision="half")
    assert len(m.state_dict()) == 150                                   # the attribute adds nothing to the checkpoint


def test_full_image_path_refuses_16_bit():
    import nerf_sos_amd
    for p in ("fp16", "bf16"):
        m = nerf_sos_amd.DinoViT(precision=p)
        with pytest.raises(ValueError, match="full-image"):
            m.get_vit_attn_feat_noresize(torch.zeros(1, 3, 64, 64))     # refused before the device of x is even looked at
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.get_vit_attn_feat(torch.zeros(1, 3, 32, 32))
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.patch_features(torch.zeros(1, 32, 32, 3), 2)


def test_ops16_refuse_fp32_and_cpu():
    from nerf_sos_amd import ops
    with pytest.raises(ValueError, match="fp16"):
        ops.dino_pack16({}, "fp32")
    with pytest.raises(ValueError, match="fp16"):
        ops.dino_forward16(torch.zeros(1, 3, 32, 32), torch.zeros(4), 0, "fp32")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_forward16(torch.zeros(1, 3, 32, 32), torch.zeros(4), 0, "bf16")
    with pytest.raises(ValueError, match="batch"):
        ops.dino_workspace16_floats(0)
    assert ops.dino_workspace16_floats(8) * 4 == _lib.lib().nsos_dino_workspace16_bytes(8)


def test_16_bit_kernels_use_no_scratch():
    """Every dino16 kernel of the built code object: no scratch instruction (the per-kernel check tests/test_abi.py runs on the MLP
    kernels), and the GEMM and attention kernels carry the 16-bit MFMA of their precision."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_lds_ring", os.path.join(ROOT, "scripts", "check_lds_ring.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert os.path.exists(chk.OBJDUMP), "llvm-objdump of the ROCm toolchain that built the library"
    kernels = {k: v for k, v in chk.disassemble(_lib.LIB_PATH).items() if "dino16_" in k}
    # per precision: prepare, layernorm, attention, round, five GEMM instantiations; + outputs, copy, add
    assert len(kernels) == 2 * 9 + 3, sorted(kernels)
    for name, ins in kernels.items():
        _, _, n_scratch = chk.check_kernel(ins)
        assert n_scratch == 0, (name, n_scratch)
        if "gemm" in name or "attention" in name:
            want = "v_mfma_f32_16x16x32_f16" if "3F16" in name else "v_mfma_f32_16x16x32_bf16"
            text = " ".join(str(i) for i in ins)
            assert want in text, (name, want)


def test_fixture_shape_and_conditions():
    g = golden16()
    assert g["meta"]["precisions"] == ["fp16", "bf16"] and g["meta"]["placements"] == ["A", "B"] and g["meta"]["outputs"] == list(fx.OUTPUTS)
    assert g["e16"].shape == (6, 2, 2, 3) and np.isfinite(g["e16"]).all() and (g["e16"] > 0).all()
    assert g["max_operand"].max() < 65504 / 16                          # fp16's range holds on the three weight kinds
    ratio = g["e16"][:, :, 1] / g["e16"][:, :, 0]
    assert 0.4 < ratio.min() and ratio.max() < 2.5                      # the two placements sample one error population
    for pi, need in ((0, 2), (1, 1)):                                   # the negatives test keeps its cases
        ok = [ci for ci in (0, 1, 2) if fx.case(ci)["gap"] > 4 * g["dsim"][ci, pi].max()]
        assert len(ok) >= need, (pi, ok)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_model_reproduces_the_committed_yardstick(precision):
    """Case 4 ([1,3,40,56], "wide") through dino16_model on this CPU against the committed e16.  Not bit-equal by design: the BLAS
    blocking and thread count change fp32 summation orders, which flips single 16-bit roundings downstream; the maximum over 75 000
    elements moves by a few percent (1 against 8 threads: under 5 %), while a changed rounding point moves it by a factor."""
    g = golden16()
    pi = g["meta"]["precisions"].index(precision)
    c = fx.case(4)
    sd = dw.make_state(c["kind"], fx.meta()["seeds"][c["kind"]])
    for li, plc in enumerate(g["meta"]["placements"]):
        o = m16.run_case(sd, c, torch.from_numpy(c["input"]), precision, plc)
        for oi, k in enumerate(fx.OUTPUTS):
            ref = c["ref64"]["feat0"][None] if k == "feat" else c["ref64"][k]
            e = float(np.abs(o[k].numpy().astype(np.float64) - ref).max())
            want = float(g["e16"][4, pi, li, oi])
            print(f"{precision} {plc} {k}: e16 here {e:.4e}, committed {want:.4e}, ratio {e / want:.3f}")
            assert 0.8 * want <= e <= 1.25 * want, (plc, k, e, want)
