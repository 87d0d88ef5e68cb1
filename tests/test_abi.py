"""CPU: the C-ABI library loads without a GPU and exports every symbol include/nerf_sos_hip.h declares;
validation paths that return before any launch behave as documented."""
import ctypes as C
import os
import re

import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "nerf_sos_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nsos_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    syms = header_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in the header but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature in _lib.py"
    assert set(_lib.SIGNATURES) == set(syms)
    declared = int(re.search(r'#define\s+NSOS_ABI_VERSION\s+(\d+)', open(os.path.join(ROOT, 'include', 'nerf_sos_hip.h')).read()).group(1))
    assert lib.nsos_abi_version() == declared == _lib.ABI_VERSION


def test_library_was_built_from_the_sources_in_the_tree():
    """A stale libnerf_sos_hip.so (or a stale object linked into it) must not pass as the current code: the library
    reports the content hash it was built under (__graft_entry__.build stamps it), compared here with the tree's."""
    import __graft_entry__ as entry
    assert _lib.built_source_hash() == entry.source_hash(), (
        "libnerf_sos_hip.so was built from other sources than the ones in the tree: run __graft_entry__.build()")


def test_packed_sizes_and_error_strings():
    lib = _lib.lib()
    # aux (1024 floats) + 73 / 77 / 78 chunk slots of 36 KiB (DESIGN.md "HBM layout")
    assert lib.nsos_mlp_packed_bytes(0) == 4 * 1024 + 73 * 36864
    assert lib.nsos_mlp_packed_bytes(1) == 4 * 1024 + 77 * 36864
    assert lib.nsos_mlp_packed_bytes(2) == 4 * 1024 + 78 * 36864
    assert lib.nsos_mlp_packed_bytes(7) == 0
    assert lib.nsos_error_string(0) == b"ok"
    assert b"NULL" in lib.nsos_error_string(-1)


def test_validation_returns_before_launch():
    lib = _lib.lib()
    null = None
    assert lib.nsos_ray_setup(null, null, null, null, 4, 64, null, null, null) == -1
    one = C.c_void_p(16)
    assert lib.nsos_ray_setup(one, one, one, null, -1, 64, one, null, null) == -2
    assert lib.nsos_ray_setup(one, one, one, null, 0, 64, one, null, null) == 0          # empty batch: no launch
    assert lib.nsos_composite(one, one, one, null, 0.0, 4, 64, 7, 0, one, one, one, one, one, one, null) == -3
    assert lib.nsos_importance_sample(one, one, null, null, 4, 513, 128, one, one, one, null, null, null) == -3   # > 512 coarse samples
    assert lib.nsos_mlp_forward_points(C.c_void_p(8), 0, one, one, 4, one, null) == -5    # misaligned packed
    assert lib.nsos_mlp_forward_points(one, 0, one, one, 0, one, null) == 0


def test_no_cpu_fallback():
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128)
    rays = torch.zeros(2, 8, 3)
    rays[1, :, 2] = -1
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        net(rays, (1.2, 14.72))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        net.nerf_fine(torch.zeros(4, 3), viewdirs=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):          # under autograd (the generic kernels' path) as well
        net.nerf_fine(torch.zeros(4, 3), viewdirs=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):          # MLP.forward on pre-encoded rows
        net.nerf.mlp(torch.zeros(4, 90))


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: nothing in the product package may import, link or load it."""
    pkg = os.path.join(ROOT, "nerf-sos_amd")
    banned = re.compile(r"import\s+oracle|from\s+oracle|liboracle|c_oracle|torch_port|nerf_oracle\.h|oracle/")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")) or f == "Makefile":
                txt = open(os.path.join(dp, f)).read()
                assert not banned.search(txt), f"{f} references oracle/"


def test_lds_ring_protocol_holds_in_the_built_code():
    """The MLP kernels wait for their inline-asm LDS reads with hand-counted lgkmcnt; hipcc may spill or copy a
    destination before its data lands (it did once, in the reduced-precision kernel).  Replay the protocol over the
    disassembled gfx950 code of the built library: no instruction may touch a still-pending read's register, and the
    kernels must stay (essentially) free of scratch traffic."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "check_lds_ring.py")
    spec = importlib.util.spec_from_file_location("check_lds_ring", path)
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    if not os.path.exists(chk.OBJDUMP):
        pytest.skip("llvm-objdump not found")
    # (mlp_generic_kernel waits for its LDS reads through the compiler's own counters: nothing hand-counted there)
    kernels = {k: v for k, v in chk.disassemble(_lib.LIB_PATH).items() if "mlp_" in k and "pack" not in k and "mlp_generic" not in k}
    assert len(kernels) >= 32, sorted(kernels)
    for name, ins in kernels.items():
        bad, n_reads, n_scratch = chk.check_kernel(ins)
        assert n_reads > 100, name
        assert not bad, (name, bad[:3])
        # the fp32 kernels are spill-free; the sem+coord reduced-precision variant keeps one 64-bit value in scratch
        # outside its MFMA chunks (harmless as long as no pending register is involved, which `bad` checks)
        limit = 0
        if "mlp_lp_kernel" in name:   # ...ELi<SEM>ELb<SAVE>E...: the training (SAVE) variant unpacks 128 words for its stores
            limit = 160 if "ELb1EEE" in name else 24   # (21 with the hardware-sine encoder)
        if "mlp_lp16_kernel" in name:  # ...ELi<SEM>ELb<SAVE>ELb<PROF>E...  every inference instantiation scratch-free; the training
            # variants keep a few dwords around their stores and ~100 spill instructions inside the never-taken ocml sincosf blocks
            # (arguments >= 2^15) of the four encoder instances
            limit = 0
            if "ELb1EEE" in name:               # PROF: diagnostics builds
                limit = 40
            if "ELb1ELb" in name:               # SAVE
                limit = 130
        if "mlp_x3_kernel" in name and "ELi0EEE" not in name:   # ...ELi<SEM>ELi<SAVE>E...: the training variants may park a
            limit = 64                                            # few row pointers / unpacked words in scratch around their stores
        assert n_scratch <= limit, (name, n_scratch)


def test_next_row_entry_points_validate_without_a_gpu():
    lib = _lib.lib()
    assert lib.nsos_eval_workspace_bytes() == 257 * 8
    assert lib.nsos_eval_postprocess(None, None, None, 0, 2, None, None, None, None, None) == 0       # empty batch
    assert lib.nsos_eval_postprocess(None, None, None, 5, 2, None, None, None, None, None) == -1      # NULL
    assert lib.nsos_corr_workspace_bytes(1, 8, 4096, 0) > 8 * 4096 * 4 * 4
    assert lib.nsos_corr_workspace_bytes(0, 8, 121, 384) > 2 * 8 * 121 * 121 * 4
    assert lib.nsos_corr_workspace_bytes(2, 8, 121, 384) == 0
    one = C.c_float(0)
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    # geometric loss: more than 4096 points per patch does not fit the LDS-resident design
    assert lib.nsos_geo_correlation_loss(p, p, p, p, p, 2, 2, 65, 64, 0.5, 1, 3, 1, 15, 1, C.byref(one), None, p, 32, None) == -3
    assert lib.nsos_geo_correlation_loss(p, p, p, p, p, 2, 5, 8, 8, 0.5, 1, 3, 1, 15, 1, C.byref(one), None, p, 32, None) == -3
    assert lib.nsos_geo_correlation_loss(p, p, p, p, p, 2, 2, 8, 8, 0.5, 1, 3, 1, 15, 1, C.byref(one), None, p, 32, None) == -4
    assert lib.nsos_app_correlation_loss(p, p, p, p, None, 2, 16, 5, 5, 2, 8, 8, 11, 0.18, 1, 0.46, 1, C.byref(one), None, p, 32, None) == -1
    assert lib.nsos_app_correlation_loss(p, p, p, p, p, 2, 16, 5, 5, 2, 8, 8, 11, 0.18, 1, 0.46, 1, C.byref(one), None, p, 32, None) == -4
    with pytest.raises(RuntimeError, match="GPU tensor"):
        nerf_sos_amd.CorrelationLoss(None)(torch.zeros(2, 4, 3, 3), torch.zeros(2, 2, 8, 8), torch.zeros(2, 2))


def test_16bit_packed_size_and_kernel_selection_without_a_gpu():
    """K2-LP, ABI 11: the packed weights hold two streams, and the selector knows two kernels (3 = mlp_lp16_kernel, 1 = mlp_lp_kernel)."""
    lib = _lib.lib()
    slot = 36 * 1024
    # [aux | mlp_lp_kernel's chunks | mlp_lp16_kernel's chunks + rgb_linear's four resident operands]: lp_chunks / lp16_chunks of csrc/lp_common.h
    for sem, (n4, n16) in enumerate([(37, 37), (39, 39), (40, 39)]):
        assert lib.nsos_mlp_packed_bytes_lp(sem) == 4096 + n4 * slot + n16 * slot + 4096
    assert lib.nsos_mlp_packed_bytes_lp(3) == 0
    prev = lib.nsos_mlp_lp_selected_kernel()
    assert prev in (1, 3)
    try:
        for k in (1, 3):
            assert lib.nsos_mlp_lp_select_kernel(k) == 0 and lib.nsos_mlp_lp_selected_kernel() == k
            for refused in (0, 2, 4):        # 2 was the retired 32x32x16 two-waves-per-SIMD kernel: refused, and the selection survives
                assert lib.nsos_mlp_lp_select_kernel(refused) == -3 and lib.nsos_mlp_lp_selected_kernel() == k
            assert lib.nsos_mlp_save16_layout(1000) == (0 if k == 1 else 16 | 32)      # both matrices row-major, or both tile-major
            assert lib.nsos_mlp_save16_layout(1 << 31) == 0                            # >= 2^31 points: the round-1 kernel
    finally:
        assert lib.nsos_mlp_lp_select_kernel(prev) == 0


@pytest.mark.parametrize("value,expect", [("lp16", 3), ("lp4", 1), ("lp8", -3), ("lp", -3), ("", -3), (None, 3)],
                         ids=["lp16", "lp4", "lp8", "lp", "empty", "unset"])
def test_lp_kernel_environment_variable(value, expect):
    """NSOS_LP_KERNEL accepts lp16 and lp4; anything else is NSOS_ERR_UNSUPPORTED from the selection and from the entries that ask
    for it (here the host-only ones; never a silent run of the default), until a kernel is selected.  In a child process: the
    variable is read once.  The child launches nothing."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import nerf_sos_amd; from nerf_sos_amd import _lib; lib = _lib.lib();"
            "print(lib.nsos_mlp_lp_selected_kernel(), lib.nsos_mlp_save16_layout(1000),"
            "      lib.nsos_mlp_lp_select_kernel(1), lib.nsos_mlp_lp_selected_kernel())" % ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("NSOS_LP_KERNEL", "NSOS_LP_WAVES")}
    if value is not None:
        env["NSOS_LP_KERNEL"] = value
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.splitlines()[-1].split()
    layout = {3: "48", 1: "0", -3: "-3"}[expect]
    assert out == [str(expect), layout, "0", "1"], out


def test_split_fp16_entry_points_validate_without_a_gpu():
    """K2-X3 / K7-X3: sizes, empty batches and argument validation are host-side (no launch)."""
    lib = _lib.lib()
    slot = 36 * 1024
    # ABI 8: [aux | mlp_x3_kernel's chunks | mlp_x316_kernel's chunks + rgb_linear's eight resident operands] (both kernels: 73 / 77 / 78 chunks)
    assert lib.nsos_mlp_packed_bytes_x3(0) == 4096 + 73 * slot + 73 * slot + 8192 and lib.nsos_mlp_packed_bytes_x3(2) == 4096 + 78 * slot + 78 * slot + 8192
    assert lib.nsos_mlp_packed_bytes_x3(1) == 4096 + 77 * slot + 77 * slot + 8192
    assert lib.nsos_mlp_packed_bytes_x3(3) == 0
    assert lib.nsos_mlp_x3_selected_kernel() in (1, 2) and lib.nsos_mlp_x3_select_kernel(3) == -3
    prev = lib.nsos_mlp_x3_selected_kernel()
    assert lib.nsos_mlp_x3_select_kernel(1) == 0 and lib.nsos_mlp_x3_selected_kernel() == 1 and lib.nsos_mlp_x3_select_kernel(prev) == 0
    assert lib.nsos_mlp_bwd_packed_bytes_x3(0) == 4096 + 68 * slot and lib.nsos_mlp_bwd_packed_bytes_x3(1) == 4096 + 72 * slot
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.nsos_mlp_forward_rays_x3(p, 0, p, p, p, p, 0, 64, p, None) == 0                 # empty batch
    assert lib.nsos_mlp_forward_rays_x3(p, 0, p, p, None, p, 4, 64, p, None) == -1             # NULL
    assert lib.nsos_mlp_forward_rays_x3(p, 3, p, p, p, p, 4, 64, p, None) == -3                # unknown semantic mode
    assert lib.nsos_mlp_forward_rays_save_x3(p, 0, p, p, p, p, 4, 64, p, p, p, None) == -3     # needs a semantic head
    assert lib.nsos_mlp_forward_rays_save_all_x3(p, 0, p, p, p, p, 4, 64, p, None, p, None) == -1
    assert lib.nsos_mlp_forward_rays_save_all_x3(p, 0, p, p, p, p, 4, 64, p, p, None, None) == -1   # the bit masks are not optional
    assert lib.nsos_mlp_relu_masks_bytes_x3(129) == 2 * 8 * 256 * 16 and lib.nsos_mlp_relu_masks_bytes_x3(0) == 0
    assert lib.nsos_mlp_input_grads_x3(p, 0, p, p, None, 0, p, p, None) == 0
    assert lib.nsos_mlp_input_grads_x3(p, 0, p, p, None, 5, None, p, None) == -1
    assert lib.nsos_mlp_bwd_pack_x3(None, 0, p, 1 << 30, None) == -1
    assert lib.nsos_sem_head_wgrad_x3(p, p, p, p, p, 0, 4, 4, p, p, p, p, p, 1 << 30, None, 0, None) == -3     # fewer than 8 samples per ray
    assert lib.nsos_sem_head_wgrad_x3(p, p, p, p, None, 0, 4, 64, None, p, p, p, p, 1 << 30, None, 0, None) == -1   # sem_in NULL (scale may be)
    assert lib.nsos_sem_head_wgrad_x3(p, p, p, p, p, 0, 4, 64, None, p, p, p, p, 1 << 20, None, 0, None) == -4      # workspace too small
    assert lib.nsos_sem_head_wgrad_x3(p, p, p, p, p, 3, 4, 64, p, p, p, p, p, 1 << 30, None, 0, None) == -3      # unknown sem_in dtype
    assert lib.nsos_mlp_forward_rays_save16_lp(p, 2, 2, p, p, p, p, 4, 64, p, None, p, None) == -1       # sem_in16 NULL
    assert lib.nsos_wgrad_x3(p, 256, p, 256, 64, None, 256, None, p, 1 << 30, None) == -1          # dW NULL
    assert lib.nsos_wgrad_x3(p, 255, p, 256, 64, p, 256, None, p, 1 << 30, None) == -2             # row stride < 256
    assert lib.nsos_wgrad_x3(p, 256, p, 256, 64, p, 256, None, p, 1024, None) == -4                # workspace too small


def test_wgrad_entry_points_refuse_before_any_launch():
    """nsos_wgrad / nsos_wgrad_xh, nsos_wgrad_batch and nsos_relu_mask: every refusal below is decided on the host (fake non-null
    pointers: nothing is dereferenced, nothing launched)."""
    lib = _lib.lib()
    NULL, SHAPE, UNSUPPORTED, SMALL, MISALIGNED = -1, -2, -3, -4, -5
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30
    for fn in (lib.nsos_wgrad, lib.nsos_wgrad_xh):
        #          G, ldg, X, ldx, n_pts, M, N, dW, ldw, db, workspace, workspace_bytes, stream
        assert fn(p, 256, p, 256, 64, 256, 256, None, 256, None, p, big, None) == NULL            # dW NULL
        assert fn(p, 256, p, 256, 64, 256, 256, p, 256, None, None, big, None) == NULL            # workspace NULL
        assert fn(p, 256, p, 256, -1, 256, 256, p, 256, None, p, big, None) == SHAPE              # n_pts < 0
        assert fn(None, 256, p, 256, 64, 256, 256, p, 256, None, p, big, None) == NULL            # G NULL with points to read
        assert fn(p, 256, None, 256, 64, 256, 256, p, 256, None, p, big, None) == NULL            # X NULL with points to read
        assert fn(p, 256, p, 256, 64, 96, 256, p, 256, None, p, big, None) == UNSUPPORTED         # M = 96
        assert fn(p, 256, p, 256, 64, 256, 48, p, 256, None, p, big, None) == UNSUPPORTED         # N = 48
        assert fn(p, 512, p, 256, 64, 512, 256, p, 256, None, p, big, None) == UNSUPPORTED        # M = 512
        assert fn(p, 127, p, 64, 64, 128, 64, p, 64, None, p, big, None) == SHAPE                 # ldg < M
        assert fn(p, 128, p, 63, 64, 128, 64, p, 64, None, p, big, None) == SHAPE                 # ldx < N
        assert fn(p, 128, p, 64, 64, 128, 64, p, 63, None, p, big, None) == SHAPE                 # ldw < N
        # workspace: blocks * KW * (M N + M) floats with blocks = min(256, ceil(n_pts / (2 KW))) -- one byte short
        assert fn(p, 32, p, 256, 20, 32, 256, p, 256, None, p, 3 * 4 * (32 * 256 + 32) * 4 - 1, None) == SMALL    # KW = 4, 3 blocks
        assert fn(p, 256, p, 256, 1 << 20, 256, 256, p, 256, None, p, 256 * (256 * 256 + 256) * 4 - 1, None) == SMALL
        assert fn(p, 32, p, 256, 1 << 20, 32, 256, p, 256, None, p, 256 * 4 * (32 * 256 + 32) * 4 - 1, None) == SMALL
    assert lib.nsos_wgrad_workspace_bytes() >= max(256 * (256 * 256 + 256) * 4, 256 * 4 * (32 * 256 + 32) * 4, 256 * 2 * (64 * 256 + 64) * 4)

    def batch(items, n_items, G=p, ldg=300, X=p, ldx=300, n_pts=64, out=p, ws=p, ws_bytes=big):
        arr = (_lib.WgradItem * max(len(items), 1))()
        for i, (w, b, gc, xc, m, n, ldw) in enumerate(items):
            arr[i].w_off, arr[i].b_off, arr[i].g_col, arr[i].x_col, arr[i].M, arr[i].N, arr[i].ldw = w, b, gc, xc, m, n, ldw
        return lib.nsos_wgrad_batch(arr if items is not None and len(items) else None, n_items, G, ldg, X, ldx, n_pts, out, ws, ws_bytes, None)

    ok = (0, -1, 0, 0, 64, 64, 64)
    assert batch([], 0) == 0 and batch([], 0, G=None, X=None, out=None, ws=None, ws_bytes=0) == 0     # an empty list is no work
    assert batch([ok], -1) == SHAPE                                                                   # n_items < 0
    assert batch([], 1) == NULL                                                                       # items NULL
    assert batch([ok], 1, out=None) == NULL
    assert batch([ok], 1, G=None) == NULL and batch([ok], 1, X=None) == NULL                          # points to read, nothing to read from
    assert batch([(0, -1, -1, 0, 64, 64, 64)], 1) == SHAPE                                            # g_col < 0
    assert batch([(0, -1, 0, -1, 64, 64, 64)], 1) == SHAPE                                            # x_col < 0
    assert batch([(-1, -1, 0, 0, 64, 64, 64)], 1) == SHAPE                                            # w_off < 0
    assert batch([(0, -1, 300 - 63, 0, 64, 64, 64)], 1) == SHAPE                                      # g_col + M > ldg
    assert batch([(0, -1, 0, 300 - 31, 64, 32, 64)], 1) == SHAPE                                      # x_col + N > ldx
    assert batch([(0, -1, 0, 0, 96, 64, 64)], 1) == UNSUPPORTED                                       # the item's own refusal: M = 96
    assert batch([(0, -1, 0, 0, 64, 64, 63)], 1) == SHAPE                                             # ... ldw < N
    assert batch([(0, -1, 0, 0, 64, 64, 64)], 1, ws_bytes=1024) == SMALL                              # ... workspace
    assert batch([(0, -1, 0, 0, 64, 64, 64)], 1, n_pts=-1) == SHAPE                                   # ... n_pts < 0

    q = C.c_void_p(p.value + 4)                                                                        # 4-byte aligned only
    assert p.value % 16 == 0
    assert lib.nsos_relu_mask(None, 0, None, 0, 0, 0, None) == 0                                       # no points: nothing to do, nothing checked
    assert lib.nsos_relu_mask(None, 64, p, 64, 8, 64, None) == NULL and lib.nsos_relu_mask(p, 64, None, 64, 8, 64, None) == NULL
    assert lib.nsos_relu_mask(p, 64, p, 64, 8, 62, None) == SHAPE                                      # n_cols not a multiple of 4
    assert lib.nsos_relu_mask(p, 64, p, 64, 8, 0, None) == SHAPE and lib.nsos_relu_mask(p, 64, p, 64, -8, 64, None) == SHAPE
    assert lib.nsos_relu_mask(p, 66, p, 64, 8, 64, None) == SHAPE and lib.nsos_relu_mask(p, 64, p, 66, 8, 64, None) == SHAPE
    assert lib.nsos_relu_mask(q, 64, p, 64, 8, 64, None) == MISALIGNED and lib.nsos_relu_mask(p, 64, q, 64, 8, 64, None) == MISALIGNED


def test_loss_entry_points_refuse_out_of_range_shapes_and_write_nothing():
    """The correlation-loss limits -- geo N = H W <= 4096 (the LDS-resident patch), code width C in 1..4 (kMaxC), appearance
    S <= 32 (S^2 <= 1024) -- are enforced before any launch: every entry returns NSOS_ERR_UNSUPPORTED and leaves the loss and
    gradient buffers as they were (host sentinels here: nothing on the device is reached)."""
    import numpy as np
    lib = _lib.lib()
    UNSUPPORTED = -3
    ws = np.zeros(64, np.float64)                 # 16-byte aligned, never touched
    arg = C.c_void_p(ws.ctypes.data)
    for case in ("geo", "geo_rows", "geo_pair", "app", "app_nhwc", "app_rows"):
        for C_, shape in ((2, (1, 4097)), (2, (17, 241)), (0, (8, 8)), (5, (8, 8)), (2, (33,)), (0, (33,)), (5, (11,))):
            geo = case.startswith("geo")
            if geo != (len(shape) == 2):
                continue
            loss = np.full(1, 1234.5, np.float32)
            grad = np.full(256, -7.25, np.float32)
            grad1 = np.full(256, -7.25, np.float32)
            L, G, G1 = (C.c_void_p(a.ctypes.data) for a in (loss, grad, grad1))
            rows = np.zeros(2, np.int32)
            R = C.c_void_p(rows.ctypes.data)
            big = 1 << 40
            if geo:
                H, W = shape
                if case == "geo":
                    rc = lib.nsos_geo_correlation_loss(arg, arg, arg, arg, arg, 2, C_, H, W, 0.5, 1, 3, 1, 15, 1, L, G, arg, big, None)
                elif case == "geo_rows":
                    rc = lib.nsos_geo_correlation_loss_rows(3, arg, arg, arg, arg, arg, R, 2, 2, C_, H, W, 0.5, 1, 3, 1, 15, 1, L, G, arg,
                                                            big, None, None, None)
                else:
                    rc = lib.nsos_geo_correlation_loss_pair(3, arg, arg, arg, arg, arg, arg, R, 2, 1, 0, C_, H, W, 0.5, 1, 3, 1, 15, L, G,
                                                            G1, arg, big, None, None, None)
            else:
                (S,) = shape
                if case == "app":
                    rc = lib.nsos_app_correlation_loss(arg, arg, arg, arg, arg, 2, 7, 5, 3, C_, 13, 20, S, 0.18, 1, 0.46, 1, L, G, arg, big, None)
                elif case == "app_nhwc":
                    rc = lib.nsos_app_correlation_loss_nhwc(arg, arg, arg, arg, arg, 2, 7, 5, 3, C_, 13, 20, S, 0.18, 1, 0.46, 1, L, G, arg, big,
                                                            None)
                else:
                    rc = lib.nsos_app_correlation_loss_rows(2, arg, arg, arg, arg, arg, R, 2, 2, 0, 7, 5, 3, C_, 13, 20, S, 0.18, 1, 0.46, 1, L,
                                                            G, arg, big, None, None, None)
            assert rc == UNSUPPORTED, (case, C_, shape, rc)
            assert loss[0] == 1234.5 and (grad == -7.25).all() and (grad1 == -7.25).all(), (case, C_, shape)
            assert (ws == 0).all()
    assert b"specialised" in lib.nsos_error_string(UNSUPPORTED)
    # the accepted boundary passes validation (and then stops at the buffer size: no launch either)
    loss = np.full(1, 1234.5, np.float32)
    L = C.c_void_p(loss.ctypes.data)
    assert lib.nsos_geo_correlation_loss(arg, arg, arg, arg, arg, 1, 4, 32, 128, 0.5, 1, 3, 1, 15, 1, L, None, arg, 32, None) == -4
    assert lib.nsos_app_correlation_loss(arg, arg, arg, arg, arg, 1, 7, 5, 3, 1, 13, 20, 32, 0.18, 1, 0.46, 1, L, None, arg, 32, None) == -4
    assert loss[0] == 1234.5


# ---- refusals of the shipped-architecture MLP entry points -----------------------------------------------------------
# Argument names in ABI order (the trailing `stream` left out).  Every case below is refused on the host: no call reaches a launch.
_RAY = ("packed", "sem_mode", "rays_o", "rays_d", "viewdirs", "z_vals", "n_rays", "n_samples", "raw")
_RAY_LP = ("packed", "sem_mode", "dtype") + _RAY[2:]
_PACK = ("T", "sem_mode", "packed", "packed_bytes")
_PACK_LP = ("T", "sem_mode", "dtype", "packed", "packed_bytes")
_POINTS = ("packed", "sem_mode", "pts", "dirs", "n_pts", "raw")
_GRADS = ("packed", "sem_mode", "g_raw", "acts", "relu_masks", "n_pts", "scale", "gbuf")
_MLP_ENTRIES = {
    "nsos_mlp_pack": _PACK, "nsos_mlp_pack_fold": _PACK, "nsos_mlp_pack_x3": _PACK, "nsos_mlp_bwd_pack_x3": _PACK,
    "nsos_mlp_pack_lp": _PACK_LP, "nsos_mlp_pack_lp_heads": _PACK_LP,
    "nsos_mlp_forward_rays": _RAY, "nsos_mlp_forward_rays_fold": _RAY,
    "nsos_mlp_forward_rays_save": _RAY + ("sem_in", "sem_hid"), "nsos_mlp_forward_rays_save_fold": _RAY + ("sem_in", "sem_hid"),
    "nsos_mlp_forward_rays_save_all": _RAY + ("acts",), "nsos_mlp_forward_rays_save_all_fold": _RAY + ("acts",),
    "nsos_mlp_forward_rays_lp": _RAY_LP, "nsos_mlp_forward_rays_save_lp": _RAY_LP + ("sem_in", "sem_hid"),
    "nsos_mlp_forward_rays_save16_lp": _RAY_LP + ("sem_in16", "sem_hid16"),
    "nsos_mlp_forward_rays_x3": _RAY, "nsos_mlp_forward_rays_save_x3": _RAY + ("sem_in", "sem_hid"),
    "nsos_mlp_forward_rays_save_all_x3": _RAY + ("acts", "relu_masks"), "nsos_mlp_forward_rays_save_all16_x3": _RAY + ("acts", "relu_masks"),
    "nsos_mlp_profile_rays": _RAY + ("stamps",), "nsos_mlp_profile_rays_fold": _RAY + ("stamps",),
    "nsos_mlp_profile_rays_lp": _RAY_LP + ("stamps",), "nsos_mlp_profile_rays_x3": _RAY + ("stamps",),
    "nsos_mlp_forward_points": _POINTS, "nsos_mlp_forward_points_fold": _POINTS,
    "nsos_mlp_input_grads_x3": _GRADS, "nsos_mlp_input_grads_x3_a16": _GRADS,
}
_SCALARS = ("sem_mode", "dtype", "n_rays", "n_samples", "n_pts", "packed_bytes")
_ALIGNED = ("packed", "raw", "gbuf", "sem_in", "sem_hid", "sem_in16", "sem_hid16", "acts", "relu_masks")   # refused unless 16-byte aligned
_NEEDS_SEM_HEAD = ("nsos_mlp_forward_rays_save", "nsos_mlp_forward_rays_save_fold", "nsos_mlp_forward_rays_save_lp",
                   "nsos_mlp_forward_rays_save16_lp", "nsos_mlp_forward_rays_save_x3", "nsos_mlp_pack_lp_heads")
_PACKED_BYTES = {"nsos_mlp_pack": "nsos_mlp_packed_bytes", "nsos_mlp_pack_fold": "nsos_mlp_packed_bytes_fold",
                 "nsos_mlp_pack_x3": "nsos_mlp_packed_bytes_x3", "nsos_mlp_bwd_pack_x3": "nsos_mlp_bwd_packed_bytes_x3",
                 "nsos_mlp_pack_lp": "nsos_mlp_packed_bytes_lp", "nsos_mlp_pack_lp_heads": "nsos_mlp_packed_bytes_lp"}
_WEIGHTS = [f"pts_w{l}" for l in range(8)] + ["alpha_w", "feature_w", "views_w", "rgb_w", "sem0_w", "sem2_w"]
_BIASES = [f"pts_b{l}" for l in range(8)] + ["alpha_b", "feature_b", "views_b", "rgb_b", "sem0_b", "sem2_b"]
# two refusals in one call: the pair's name is "<first> + <second>", each a single case of the entry point
_PAIRS = [("null:raw", "sem_mode:3"), ("misaligned:raw", "n_rays:2^31"), ("sem_mode:3", "misaligned:packed"), ("n_samples:0", "null:rays_o"),
          ("dtype:3", "n_samples:0"), ("dtype:3", "misaligned:raw"), ("dtype:3", "n_rays:2^31"), ("null:sem_in", "misaligned:packed"),
          ("null:sem_hid", "n_samples:0"), ("sem_mode:0", "null:sem_in"), ("sem_mode:0", "misaligned:sem_hid"), ("sem_mode:0", "misaligned:raw"),
          ("sem_mode:3", "misaligned:sem_in"), ("null:acts", "sem_mode:3"), ("misaligned:acts", "null:raw"), ("misaligned:acts", "n_samples:0"),
          ("null:relu_masks", "misaligned:raw"), ("misaligned:relu_masks", "tiles:2^31"), ("null:stamps", "null:packed"),
          ("null:stamps", "sem_mode:3"), ("null:sem_in16", "dtype:3"), ("misaligned:sem_hid16", "null:z_vals"),
          ("tiles:2^31", "misaligned:raw"), ("tiles:2^31", "sem_mode:3"), ("n_rays:2^31", "sem_mode:3"), ("n_rays:-1", "null:packed"),
          ("n_rays:-1", "misaligned:packed"), ("n_pts:2^39", "misaligned:raw"), ("n_pts:2^39", "misaligned:gbuf"), ("n_pts:-1", "null:raw"),
          ("n_pts:-1", "sem_mode:3"), ("sem_mode:3", "n_pts:2^39"), ("sem_mode:3", "misaligned:acts"), ("null:T", "sem_mode:3"),
          ("sem_mode:3", "packed_bytes:short"), ("packed_bytes:short", "misaligned:packed"), ("misaligned:packed", "null:T.rgb_w"),
          ("dtype:3", "packed_bytes:short"), ("dtype:0", "null:packed"), ("sem_mode:0", "null:T"), ("sem_mode:0", "packed_bytes:short"),
          ("packed_bytes:short", "null:T.pts_w3")]


def _mlp_refusal_cases(lib, name):
    """{case: {argument: value}}: what to change in an otherwise valid call of `name` (sem+coord net, fp16, 4 rays x 64 samples)."""
    args = _MLP_ENTRIES[name]
    ptrs = [a for a in args if a not in _SCALARS and a != "T"]
    optional = ["relu_masks"] if name == "nsos_mlp_input_grads_x3" else []
    count = "n_rays" if "n_rays" in args else "n_pts"
    cases = {}
    if "T" in args:
        fields = _WEIGHTS[1:] if name == "nsos_mlp_bwd_pack_x3" else _WEIGHTS + _BIASES   # the backward packs no bias and not layer 0
        cases.update({"null:T": {"T": None}, "packed_bytes:0": {"packed_bytes": 0},
                      "packed_bytes:short": {"packed_bytes": getattr(lib, _PACKED_BYTES[name])(2) - 1}})
        cases.update({f"null:T.{f}": {"T": f} for f in fields})
    else:
        cases["zero"] = dict({a: None for a in ptrs}, **{count: 0})
        cases[f"{count}:-1"] = {count: -1}
    cases.update({f"null:{a}": {a: None} for a in ptrs if a not in optional})
    cases.update({f"misaligned:{a}": {a: "odd"} for a in ptrs if a in _ALIGNED})
    cases["sem_mode:3"] = {"sem_mode": 3}
    if name in _NEEDS_SEM_HEAD:
        cases["sem_mode:0"] = {"sem_mode": 0}
    if "dtype" in args:
        cases.update({"dtype:0": {"dtype": 0}, "dtype:3": {"dtype": 3}})
    if "n_rays" in args:
        cases["n_samples:0"] = {"n_samples": 0}
        cases["n_rays:2^31"] = {"n_rays": 1 << 31, "n_samples": 128}          # 2^31 tiles as well, for the entry points that take 2^31 rays
        cases["tiles:2^31"] = {"n_rays": (1 << 31) - 1, "n_samples": (1 << 31) - 1}
    if "n_pts" in args:
        cases["n_pts:2^39"] = {"n_pts": 1 << 39}                              # 2^32 tiles of 128 points
    for a, b in _PAIRS:
        if a in cases and b in cases and not set(cases[a]) & set(cases[b]):
            cases[f"{a} + {b}"] = dict(cases[a], **cases[b])
    return cases


def _call_mlp_entry(lib, name, change, buf):
    """`name` with valid arguments except for `change`.  Pointers are host addresses inside `buf`: nothing may dereference them."""
    base = C.addressof(buf)
    assert base % 16 == 0
    value = {"sem_mode": 2, "dtype": 1, "n_rays": 4, "n_samples": 64, "n_pts": 256, "packed_bytes": 1 << 30}
    call = []
    for a in _MLP_ENTRIES[name]:
        v = change.get(a, value.get(a, base))
        if a == "T" and v is not None:
            t = _lib.MlpTensors()
            for f in _WEIGHTS + _BIASES:
                p = None if f == v else base
                if f.startswith("pts_"):
                    getattr(t, f[:5])[int(f[5])] = p
                else:
                    setattr(t, f, p)
            v = C.byref(t)
        elif v == "odd":
            v = base + 8
        call.append(v)
    return getattr(lib, name)(*call, None)


# Return codes of the library as it was before mlp_host.h took over the host-side checks (recorded from a build of that commit):
# 0 ok, -1 NULL pointer, -2 bad shape, -3 unsupported, -4 buffer too small, -5 misaligned.
_MLP_REFUSALS = {}
for _names, _row in (
    (("nsos_mlp_pack", "nsos_mlp_pack_fold", "nsos_mlp_pack_x3",), {
        "null:T": -1, "packed_bytes:0": -4, "packed_bytes:short": -4, "null:T.pts_w0": -1, "null:T.pts_w1": -1, "null:T.pts_w2": -1,
        "null:T.pts_w3": -1, "null:T.pts_w4": -1, "null:T.pts_w5": -1, "null:T.pts_w6": -1, "null:T.pts_w7": -1,
        "null:T.alpha_w": -1, "null:T.feature_w": -1, "null:T.views_w": -1, "null:T.rgb_w": -1, "null:T.sem0_w": -1,
        "null:T.sem2_w": -1, "null:T.pts_b0": -1, "null:T.pts_b1": -1, "null:T.pts_b2": -1, "null:T.pts_b3": -1,
        "null:T.pts_b4": -1, "null:T.pts_b5": -1, "null:T.pts_b6": -1, "null:T.pts_b7": -1, "null:T.alpha_b": -1,
        "null:T.feature_b": -1, "null:T.views_b": -1, "null:T.rgb_b": -1, "null:T.sem0_b": -1, "null:T.sem2_b": -1,
        "null:packed": -1, "misaligned:packed": -5, "sem_mode:3": -3, "sem_mode:3 + misaligned:packed": -3,
        "null:T + sem_mode:3": -1, "sem_mode:3 + packed_bytes:short": -3, "packed_bytes:short + misaligned:packed": -4,
        "misaligned:packed + null:T.rgb_w": -5, "packed_bytes:short + null:T.pts_w3": -4,
    }),
    (("nsos_mlp_bwd_pack_x3",), {
        "null:T": -1, "packed_bytes:0": -4, "packed_bytes:short": -4, "null:T.pts_w1": -1, "null:T.pts_w2": -1, "null:T.pts_w3": -1,
        "null:T.pts_w4": -1, "null:T.pts_w5": -1, "null:T.pts_w6": -1, "null:T.pts_w7": -1, "null:T.alpha_w": -1,
        "null:T.feature_w": -1, "null:T.views_w": -1, "null:T.rgb_w": -1, "null:T.sem0_w": -1, "null:T.sem2_w": -1,
        "null:packed": -1, "misaligned:packed": -5, "sem_mode:3": -3, "sem_mode:3 + misaligned:packed": -3,
        "null:T + sem_mode:3": -1, "sem_mode:3 + packed_bytes:short": -3, "packed_bytes:short + misaligned:packed": -4,
        "misaligned:packed + null:T.rgb_w": -5, "packed_bytes:short + null:T.pts_w3": -4,
    }),
    (("nsos_mlp_pack_lp",), {
        "null:T": -1, "packed_bytes:0": -4, "packed_bytes:short": -4, "null:T.pts_w0": -1, "null:T.pts_w1": -1, "null:T.pts_w2": -1,
        "null:T.pts_w3": -1, "null:T.pts_w4": -1, "null:T.pts_w5": -1, "null:T.pts_w6": -1, "null:T.pts_w7": -1,
        "null:T.alpha_w": -1, "null:T.feature_w": -1, "null:T.views_w": -1, "null:T.rgb_w": -1, "null:T.sem0_w": -1,
        "null:T.sem2_w": -1, "null:T.pts_b0": -1, "null:T.pts_b1": -1, "null:T.pts_b2": -1, "null:T.pts_b3": -1,
        "null:T.pts_b4": -1, "null:T.pts_b5": -1, "null:T.pts_b6": -1, "null:T.pts_b7": -1, "null:T.alpha_b": -1,
        "null:T.feature_b": -1, "null:T.views_b": -1, "null:T.rgb_b": -1, "null:T.sem0_b": -1, "null:T.sem2_b": -1,
        "null:packed": -1, "misaligned:packed": -5, "sem_mode:3": -3, "dtype:0": -3, "dtype:3": -3,
        "sem_mode:3 + misaligned:packed": -3, "null:T + sem_mode:3": -1, "sem_mode:3 + packed_bytes:short": -3,
        "packed_bytes:short + misaligned:packed": -4, "misaligned:packed + null:T.rgb_w": -5, "dtype:3 + packed_bytes:short": -3,
        "dtype:0 + null:packed": -1, "packed_bytes:short + null:T.pts_w3": -4,
    }),
    (("nsos_mlp_pack_lp_heads",), {
        "null:T": -1, "packed_bytes:0": -4, "packed_bytes:short": -4, "null:T.pts_w0": -1, "null:T.pts_w1": -1, "null:T.pts_w2": -1,
        "null:T.pts_w3": -1, "null:T.pts_w4": -1, "null:T.pts_w5": -1, "null:T.pts_w6": -1, "null:T.pts_w7": -1,
        "null:T.alpha_w": -1, "null:T.feature_w": -1, "null:T.views_w": -1, "null:T.rgb_w": -1, "null:T.sem0_w": -1,
        "null:T.sem2_w": -1, "null:T.pts_b0": -1, "null:T.pts_b1": -1, "null:T.pts_b2": -1, "null:T.pts_b3": -1,
        "null:T.pts_b4": -1, "null:T.pts_b5": -1, "null:T.pts_b6": -1, "null:T.pts_b7": -1, "null:T.alpha_b": -1,
        "null:T.feature_b": -1, "null:T.views_b": -1, "null:T.rgb_b": -1, "null:T.sem0_b": -1, "null:T.sem2_b": -1,
        "null:packed": -1, "misaligned:packed": -5, "sem_mode:3": -3, "sem_mode:0": -3, "dtype:0": -3, "dtype:3": -3,
        "sem_mode:3 + misaligned:packed": -3, "null:T + sem_mode:3": -3, "sem_mode:3 + packed_bytes:short": -3,
        "packed_bytes:short + misaligned:packed": -4, "misaligned:packed + null:T.rgb_w": -5, "dtype:3 + packed_bytes:short": -3,
        "dtype:0 + null:packed": -1, "sem_mode:0 + null:T": -3, "sem_mode:0 + packed_bytes:short": -3,
        "packed_bytes:short + null:T.pts_w3": -4,
    }),
    (("nsos_mlp_forward_rays", "nsos_mlp_forward_rays_fold",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "misaligned:packed": -5, "misaligned:raw": -5, "sem_mode:3": -3, "n_samples:0": -2, "n_rays:2^31": -3,
        "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -5, "sem_mode:3 + misaligned:packed": -5,
        "n_samples:0 + null:rays_o": -1, "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3,
        "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2,
    }),
    (("nsos_mlp_forward_rays_save", "nsos_mlp_forward_rays_save_fold",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:sem_in": -1, "null:sem_hid": -1, "misaligned:packed": -5, "misaligned:raw": -5,
        "misaligned:sem_in": -5, "misaligned:sem_hid": -5, "sem_mode:3": -3, "sem_mode:0": -3, "n_samples:0": -2, "n_rays:2^31": -3,
        "tiles:2^31": -3, "null:raw + sem_mode:3": -3, "misaligned:raw + n_rays:2^31": -5, "sem_mode:3 + misaligned:packed": -3,
        "n_samples:0 + null:rays_o": -1, "null:sem_in + misaligned:packed": -1, "null:sem_hid + n_samples:0": -1,
        "sem_mode:0 + null:sem_in": -1, "sem_mode:0 + misaligned:sem_hid": -3, "sem_mode:0 + misaligned:raw": -3,
        "sem_mode:3 + misaligned:sem_in": -3, "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3,
        "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2,
    }),
    (("nsos_mlp_forward_rays_save_all", "nsos_mlp_forward_rays_save_all_fold",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:acts": -1, "misaligned:packed": -5, "misaligned:raw": -5, "misaligned:acts": -5, "sem_mode:3": -3,
        "n_samples:0": -2, "n_rays:2^31": -3, "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -5,
        "sem_mode:3 + misaligned:packed": -5, "n_samples:0 + null:rays_o": -1, "null:acts + sem_mode:3": -1,
        "misaligned:acts + null:raw": -5, "misaligned:acts + n_samples:0": -5, "tiles:2^31 + misaligned:raw": -5,
        "tiles:2^31 + sem_mode:3": -3, "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1,
        "n_rays:-1 + misaligned:packed": -2, "sem_mode:3 + misaligned:acts": -5,
    }),
    (("nsos_mlp_forward_rays_lp",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "misaligned:packed": -5, "misaligned:raw": -5, "sem_mode:3": -3, "dtype:0": -3, "dtype:3": -3,
        "n_samples:0": -2, "n_rays:2^31": -3, "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -3,
        "sem_mode:3 + misaligned:packed": -3, "n_samples:0 + null:rays_o": -1, "dtype:3 + n_samples:0": -2,
        "dtype:3 + misaligned:raw": -3, "dtype:3 + n_rays:2^31": -3, "tiles:2^31 + misaligned:raw": -5,
        "tiles:2^31 + sem_mode:3": -3, "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1,
        "n_rays:-1 + misaligned:packed": -2, "dtype:0 + null:packed": -1,
    }),
    (("nsos_mlp_forward_rays_save_lp",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:sem_in": -1, "null:sem_hid": -1, "misaligned:packed": -5, "misaligned:raw": -5,
        "misaligned:sem_in": -5, "misaligned:sem_hid": -5, "sem_mode:3": -3, "sem_mode:0": -3, "dtype:0": -3, "dtype:3": -3,
        "n_samples:0": -2, "n_rays:2^31": -3, "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -3,
        "sem_mode:3 + misaligned:packed": -3, "n_samples:0 + null:rays_o": -1, "dtype:3 + n_samples:0": -2,
        "dtype:3 + misaligned:raw": -3, "dtype:3 + n_rays:2^31": -3, "null:sem_in + misaligned:packed": -1,
        "null:sem_hid + n_samples:0": -1, "sem_mode:0 + null:sem_in": -1, "sem_mode:0 + misaligned:sem_hid": -5,
        "sem_mode:0 + misaligned:raw": -5, "sem_mode:3 + misaligned:sem_in": -5, "tiles:2^31 + misaligned:raw": -5,
        "tiles:2^31 + sem_mode:3": -3, "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1,
        "n_rays:-1 + misaligned:packed": -2, "dtype:0 + null:packed": -1,
    }),
    (("nsos_mlp_forward_rays_save16_lp",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:sem_in16": -1, "null:sem_hid16": -1, "misaligned:packed": -5, "misaligned:raw": -5,
        "misaligned:sem_in16": -5, "misaligned:sem_hid16": -5, "sem_mode:3": -3, "sem_mode:0": -3, "dtype:0": -3, "dtype:3": -3,
        "n_samples:0": -2, "n_rays:2^31": -3, "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -3,
        "sem_mode:3 + misaligned:packed": -3, "n_samples:0 + null:rays_o": -1, "dtype:3 + n_samples:0": -2,
        "dtype:3 + misaligned:raw": -3, "dtype:3 + n_rays:2^31": -3, "sem_mode:0 + misaligned:raw": -5,
        "null:sem_in16 + dtype:3": -1, "misaligned:sem_hid16 + null:z_vals": -5, "tiles:2^31 + misaligned:raw": -5,
        "tiles:2^31 + sem_mode:3": -3, "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1,
        "n_rays:-1 + misaligned:packed": -2, "dtype:0 + null:packed": -1,
    }),
    (("nsos_mlp_forward_rays_x3",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "misaligned:packed": -5, "misaligned:raw": -5, "sem_mode:3": -3, "n_samples:0": -2, "n_rays:2^31": -3,
        "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -3, "sem_mode:3 + misaligned:packed": -3,
        "n_samples:0 + null:rays_o": -1, "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3,
        "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2,
    }),
    (("nsos_mlp_forward_rays_save_x3",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:sem_in": -1, "null:sem_hid": -1, "misaligned:packed": -5, "misaligned:raw": -5,
        "misaligned:sem_in": -5, "misaligned:sem_hid": -5, "sem_mode:3": -3, "sem_mode:0": -3, "n_samples:0": -2, "n_rays:2^31": -3,
        "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -3, "sem_mode:3 + misaligned:packed": -3,
        "n_samples:0 + null:rays_o": -1, "null:sem_in + misaligned:packed": -5, "null:sem_hid + n_samples:0": -2,
        "sem_mode:0 + null:sem_in": -3, "sem_mode:0 + misaligned:sem_hid": -3, "sem_mode:0 + misaligned:raw": -5,
        "sem_mode:3 + misaligned:sem_in": -3, "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3,
        "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2,
    }),
    (("nsos_mlp_forward_rays_save_all_x3", "nsos_mlp_forward_rays_save_all16_x3",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:acts": -1, "null:relu_masks": -1, "misaligned:packed": -5, "misaligned:raw": -5,
        "misaligned:acts": -5, "misaligned:relu_masks": -5, "sem_mode:3": -3, "n_samples:0": -2, "n_rays:2^31": -3,
        "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -3, "sem_mode:3 + misaligned:packed": -3,
        "n_samples:0 + null:rays_o": -1, "null:acts + sem_mode:3": -3, "misaligned:acts + null:raw": -1,
        "misaligned:acts + n_samples:0": -2, "null:relu_masks + misaligned:raw": -5, "misaligned:relu_masks + tiles:2^31": -5,
        "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3, "n_rays:2^31 + sem_mode:3": -3,
        "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2, "sem_mode:3 + misaligned:acts": -3,
    }),
    (("nsos_mlp_profile_rays", "nsos_mlp_profile_rays_fold",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:stamps": -1, "misaligned:packed": -5, "misaligned:raw": -5, "sem_mode:3": -3, "n_samples:0": -2,
        "n_rays:2^31": -3, "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -5,
        "sem_mode:3 + misaligned:packed": -5, "n_samples:0 + null:rays_o": -1, "null:stamps + null:packed": -1,
        "null:stamps + sem_mode:3": -1, "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3,
        "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2,
    }),
    (("nsos_mlp_profile_rays_lp",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:stamps": -1, "misaligned:packed": -5, "misaligned:raw": -5, "sem_mode:3": -3, "dtype:0": -3,
        "dtype:3": -3, "n_samples:0": -2, "n_rays:2^31": -3, "tiles:2^31": -3, "null:raw + sem_mode:3": -1,
        "misaligned:raw + n_rays:2^31": -3, "sem_mode:3 + misaligned:packed": -3, "n_samples:0 + null:rays_o": -1,
        "dtype:3 + n_samples:0": -2, "dtype:3 + misaligned:raw": -3, "dtype:3 + n_rays:2^31": -3, "null:stamps + null:packed": -1,
        "null:stamps + sem_mode:3": -1, "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3,
        "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2,
        "dtype:0 + null:packed": -1,
    }),
    (("nsos_mlp_profile_rays_x3",), {
        "zero": 0, "n_rays:-1": -2, "null:packed": -1, "null:rays_o": -1, "null:rays_d": -1, "null:viewdirs": -1, "null:z_vals": -1,
        "null:raw": -1, "null:stamps": -1, "misaligned:packed": -5, "misaligned:raw": -5, "sem_mode:3": -3, "n_samples:0": -2,
        "n_rays:2^31": -3, "tiles:2^31": -3, "null:raw + sem_mode:3": -1, "misaligned:raw + n_rays:2^31": -3,
        "sem_mode:3 + misaligned:packed": -3, "n_samples:0 + null:rays_o": -1, "null:stamps + null:packed": -1,
        "null:stamps + sem_mode:3": -1, "tiles:2^31 + misaligned:raw": -5, "tiles:2^31 + sem_mode:3": -3,
        "n_rays:2^31 + sem_mode:3": -3, "n_rays:-1 + null:packed": -1, "n_rays:-1 + misaligned:packed": -2,
    }),
    (("nsos_mlp_forward_points", "nsos_mlp_forward_points_fold",), {
        "zero": 0, "n_pts:-1": -2, "null:packed": -1, "null:pts": -1, "null:dirs": -1, "null:raw": -1, "misaligned:packed": -5,
        "misaligned:raw": -5, "sem_mode:3": -3, "n_pts:2^39": -3, "null:raw + sem_mode:3": -1, "sem_mode:3 + misaligned:packed": -5,
        "n_pts:2^39 + misaligned:raw": -5, "n_pts:-1 + null:raw": -1, "n_pts:-1 + sem_mode:3": -2, "sem_mode:3 + n_pts:2^39": -3,
    }),
    (("nsos_mlp_input_grads_x3",), {
        "zero": 0, "n_pts:-1": -2, "null:packed": -1, "null:g_raw": -1, "null:acts": -1, "null:scale": -1, "null:gbuf": -1,
        "misaligned:packed": -5, "misaligned:acts": -5, "misaligned:relu_masks": -5, "misaligned:gbuf": -5, "sem_mode:3": -3,
        "n_pts:2^39": -3, "sem_mode:3 + misaligned:packed": -3, "null:acts + sem_mode:3": -1, "n_pts:2^39 + misaligned:gbuf": -5,
        "n_pts:-1 + sem_mode:3": -2, "sem_mode:3 + n_pts:2^39": -3, "sem_mode:3 + misaligned:acts": -3,
    }),
    (("nsos_mlp_input_grads_x3_a16",), {
        "zero": 0, "n_pts:-1": -2, "null:packed": -1, "null:g_raw": -1, "null:acts": -1, "null:relu_masks": -1, "null:scale": -1,
        "null:gbuf": -1, "misaligned:packed": -5, "misaligned:acts": -5, "misaligned:relu_masks": -5, "misaligned:gbuf": -5,
        "sem_mode:3": -3, "n_pts:2^39": -3, "sem_mode:3 + misaligned:packed": -3, "null:acts + sem_mode:3": -1,
        "n_pts:2^39 + misaligned:gbuf": -5, "n_pts:-1 + sem_mode:3": -2, "sem_mode:3 + n_pts:2^39": -3,
        "sem_mode:3 + misaligned:acts": -3,
    }),
):
    _MLP_REFUSALS.update({_n: _row for _n in _names})


def test_mlp_entry_points_refuse_what_they_refused_before():
    """Every shipped-architecture MLP entry point, every way of getting a call wrong, and pairs of them (which pin the ORDER of the
    checks): the codes are literals taken from the library before the checks were shared.  All calls return before a launch."""
    lib = _lib.lib()
    buf = (C.c_double * 8)()
    assert set(_MLP_REFUSALS) == set(_MLP_ENTRIES)
    n = 0
    for name in _MLP_ENTRIES:
        cases = _mlp_refusal_cases(lib, name)
        assert set(cases) == set(_MLP_REFUSALS[name]), (name, set(cases) ^ set(_MLP_REFUSALS[name]))
        for case, change in cases.items():
            want = _MLP_REFUSALS[name][case]
            assert (want == 0) == (case == "zero"), (name, case)       # only the empty batch is accepted
            assert _call_mlp_entry(lib, name, change, buf) == want, (name, case)
            n += 1
    assert n > 700


# ---- refusals of the six correlation-loss entry points ----------------------------------------------------------------
# Argument names in ABI order.  A name that _LOSS_BASE does not list is a pointer: non-NULL and 16-byte aligned by default.
_F4 = ("self_shift", "self_weight", "neg_shift", "neg_weight")
_GEO_TAIL = ("workspace", "workspace_bytes", "exchange_means", "exchange_sums", "stream")
_APP_DIMS = ("feat_dim", "feat_h", "feat_w", "code_dim", "code_h", "code_w", "feature_samples")
_APP = (("feats", "code", "neg", "rand1", "rand2", "batch") + _APP_DIMS + _F4 + ("loss", "grad", "workspace", "workspace_bytes", "stream"))
_LOSS_ENTRIES = {
    "nsos_geo_correlation_loss": ("depth", "code", "ray_o", "ray_d", "neg", "batch", "code_dim", "height", "width") + _F4
                                 + ("max_depth", "filter_in_place", "loss", "grad", "workspace", "workspace_bytes", "stream"),
    "nsos_geo_correlation_loss_rows": ("phase", "depth", "code", "ray_o", "ray_d", "neg", "rows", "n_rows", "batch", "code_dim", "height",
                                       "width") + _F4 + ("max_depth", "filter_in_place", "loss", "grad") + _GEO_TAIL,
    "nsos_geo_correlation_loss_pair": ("phase", "depth", "code", "code1", "ray_o", "ray_d", "neg", "rows", "n_rows", "batch", "channel_last",
                                       "code_dim", "height", "width") + _F4 + ("max_depth", "loss", "grad", "grad1") + _GEO_TAIL,
    "nsos_app_correlation_loss": _APP,
    "nsos_app_correlation_loss_nhwc": _APP,
    "nsos_app_correlation_loss_rows": ("phase", "feats", "code", "neg", "rand1", "rand2", "rows", "n_rows", "batch", "channel_last") + _APP_DIMS
                                      + _F4 + ("loss", "grad") + _GEO_TAIL,
}
_LOSS_BASE = dict(batch=2, n_rows=2, channel_last=0, code_dim=2, height=8, width=8, feat_dim=7, feat_h=5, feat_w=3, code_h=13, code_w=20,
                  feature_samples=11, self_shift=0.5, self_weight=1.0, neg_shift=3.0, neg_weight=1.0, max_depth=15.0, filter_in_place=1,
                  exchange_means=None, exchange_sums=None, stream=None)
_LAST_PHASE = {"nsos_geo_correlation_loss_rows": 3, "nsos_geo_correlation_loss_pair": 3, "nsos_app_correlation_loss_rows": 2}


class _Off(int):
    """a pointer argument this many bytes behind the aligned buffer"""


_NULL_, _SHAPE_, _UNSUP_, _SMALL_, _MISAL_ = -1, -2, -3, -4, -5
# The base call is right in everything but `workspace_bytes`, which is ONE short of nsos_corr_workspace_bytes(...): the last check of
# every entry, so the base call returns _SMALL_ without a launch and every earlier fault shows through it.  Each row: what is changed
# in the base call -> the code, a literal read off the entry points before their checks were shared (and confirmed on that library).
_GEO_COMMON = [
    (dict(grad=None), _SMALL_),                                            # the gradient is optional
    (dict(height=0), _SHAPE_), (dict(width=0), _SHAPE_),
    (dict(code_dim=0), _UNSUP_), (dict(code_dim=5), _UNSUP_),
    (dict(height=65, width=64), _UNSUP_),                                  # N = 4160 > 4096
    (dict(workspace=_Off(8)), _MISAL_),
    (dict(), _SMALL_),                                                     # workspace_bytes one short
    (dict(code_dim=5, workspace_bytes=0), _UNSUP_),                        # two faults: the code width is checked before the size
    (dict(height=65, width=64, workspace=_Off(8)), _UNSUP_),               # ... N before the workspace's alignment
    (dict(depth=None, height=0), _NULL_),                                  # ... pointers before shapes
]
_ROWS_COMMON = [                                                           # the four entries with phases, rows and exchange buffers
    (dict(phase=-1), _UNSUP_),
    (dict(rows=None), _NULL_), (dict(rows=None, n_rows=0), _SMALL_),       # no rows: no list needed
    (dict(phase=0, loss=None), _SMALL_), (dict(phase=1, loss=None), _SMALL_), (dict(phase=2, loss=None), _NULL_),
    (dict(n_rows=-1), _SHAPE_),
    (dict(exchange_means=_Off(0), exchange_sums=_Off(0)), _SMALL_),
    (dict(exchange_means=_Off(4)), _MISAL_), (dict(exchange_sums=_Off(2)), _MISAL_),
]
_GEO_ROWS_COMMON = _GEO_COMMON + _ROWS_COMMON + [
    (dict(phase=4), _UNSUP_), (dict(phase=3, loss=None), _NULL_),
    (dict(phase=4, depth=None), _UNSUP_),                                  # two faults: the phase comes first,
    (dict(exchange_means=_Off(4), depth=None), _MISAL_),                   # then the exchange buffers' alignment, then the pointers
    (dict(exchange_sums=_Off(2), rows=None), _MISAL_),
    (dict(exchange_means=_Off(4), code_dim=5), _MISAL_),
    (dict(loss=None, height=0), _NULL_),
]
_APP_COMMON = [
    (dict(grad=None), _SMALL_),
    (dict(feat_dim=0), _SHAPE_), (dict(feat_h=0), _SHAPE_), (dict(feat_w=0), _SHAPE_), (dict(code_h=0), _SHAPE_), (dict(code_w=0), _SHAPE_),
    (dict(feature_samples=0), _SHAPE_), (dict(batch=-1), _SHAPE_),
    (dict(code_dim=0), _UNSUP_), (dict(code_dim=5), _UNSUP_),
    (dict(feature_samples=33), _UNSUP_),                                   # S^2 = 1089 > 1024
    (dict(workspace=_Off(8)), _MISAL_),
    (dict(), _SMALL_),
    (dict(code_dim=5, workspace_bytes=0), _UNSUP_),
    (dict(feature_samples=33, workspace=_Off(8)), _UNSUP_),
    (dict(feats=None, feat_h=0), _NULL_),
]
_LOSS_REFUSALS = {
    "nsos_geo_correlation_loss": _GEO_COMMON + [
        (dict(batch=-1), _SHAPE_), (dict(loss=None), _NULL_),
    ] + [({k: None}, _NULL_) for k in ("depth", "code", "ray_o", "ray_d", "neg", "workspace")],
    "nsos_geo_correlation_loss_rows": _GEO_ROWS_COMMON + [
        (dict(batch=-1), _SHAPE_), (dict(n_rows=3), _SHAPE_),
        (dict(batch=-1, phase=4), _UNSUP_),                                # the phase before the batch ...
    ] + [({k: None}, _NULL_) for k in ("depth", "code", "ray_o", "ray_d", "neg", "workspace")],
    "nsos_geo_correlation_loss_pair": _GEO_ROWS_COMMON + [
        (dict(grad1=None), _SMALL_),
        (dict(batch=-1), _SHAPE_), (dict(n_rows=4), _SMALL_), (dict(n_rows=5), _SHAPE_),     # two code maps: 2 * batch row patches
        (dict(batch=-1, phase=4), _SHAPE_),                                # ... here the batch before the phase
    ] + [({k: None}, _NULL_) for k in ("depth", "code", "code1", "ray_o", "ray_d", "neg", "workspace")],
    "nsos_app_correlation_loss": _APP_COMMON + [(dict(loss=None), _NULL_)]
                                 + [({k: None}, _NULL_) for k in ("feats", "code", "neg", "rand1", "rand2", "workspace")],
    "nsos_app_correlation_loss_nhwc": _APP_COMMON + [(dict(loss=None), _NULL_)]
                                      + [({k: None}, _NULL_) for k in ("feats", "code", "neg", "rand1", "rand2", "workspace")],
    "nsos_app_correlation_loss_rows": _APP_COMMON + _ROWS_COMMON + [
        (dict(phase=3), _UNSUP_), (dict(n_rows=3), _SHAPE_),
        (dict(phase=3, feats=None), _UNSUP_),                              # two faults: the phase first, then -- unlike the geometric
        (dict(exchange_means=_Off(4), feats=None), _NULL_),                # entries -- pointers, shapes and limits, and only then the
        (dict(exchange_sums=_Off(2), rows=None), _NULL_),                  # alignment of workspace and exchange buffers together
        (dict(exchange_means=_Off(4), code_dim=5), _UNSUP_),
        (dict(exchange_means=_Off(4), n_rows=3), _SHAPE_),
        (dict(batch=-1, phase=3), _UNSUP_),
    ] + [({k: None}, _NULL_) for k in ("feats", "code", "neg", "rand1", "rand2", "workspace")],
}


def test_loss_entry_points_report_the_same_fault_first():
    """All six correlation-loss entry points: every single way of getting a call wrong, and pairs of faults (which pin the ORDER of the
    checks).  Validation precedes any HIP call: nothing is launched, no device is needed."""
    lib = _lib.lib()
    buf = (C.c_double * 8)()
    base_ptr = C.cast(buf, C.c_void_p).value
    assert base_ptr % 16 == 0
    assert set(_LOSS_REFUSALS) == set(_LOSS_ENTRIES)
    n = 0
    for name, argnames in _LOSS_ENTRIES.items():
        geo, pair = "geo" in name, name.endswith("_pair")
        full = (lib.nsos_corr_workspace_bytes(1, 4 if pair else 2, 64, 0) if geo else lib.nsos_corr_workspace_bytes(0, 2, 121, 7))
        assert full > 0

        def call(change):
            vals = dict(_LOSS_BASE, phase=_LAST_PHASE.get(name, 0), workspace_bytes=full - 1)
            vals.update(change)
            args = []
            for a in argnames:
                v = vals.get(a, _Off(0))
                args.append(C.c_void_p(base_ptr + v) if isinstance(v, _Off) else v)
            return getattr(lib, name)(*args)

        for change, want in _LOSS_REFUSALS[name]:
            assert call(change) == want, (name, change, want)
            n += 1
        # an empty batch is no work: accepted whatever else the call holds
        empty = {a: (None if a not in _LOSS_BASE and a not in ("phase", "workspace_bytes") else 0) for a in argnames}
        empty.update(code_dim=5, phase=9, n_rows=7, stream=None)
        assert call({k: v for k, v in empty.items() if k in argnames}) == 0, name
    assert n > 150
