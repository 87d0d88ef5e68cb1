"""GPU (-m gpu): the folded fp32 stream (feature_linear multiplied into views_linears.0 at pack time; DESIGN.md "View fold").

What is held here:
  * folded against unfolded at the ops level: sigma / semantics bit-identical, rgb inside the 5e-6 band the unfolded kernel is
    granted against the C oracle (tests/test_gpu_parity.py::test_mlp_points_golden) -- seed-0 nets of every config, peaky and
    not, and the trained field on rays of its own scene; both chains' distance to an fp64 evaluation is printed;
  * at x = 0, dir = 0 (no libm) the folded kernel equals, bit for bit, an emulation written here: W' and b' by sequential fp64
    multiply-then-add with one rounding, the view layer's fp32 fma chain in the kernel's k order, the rgb head as the oracle's
    dot_halves; W' and b' read back from the packed buffer equal the numpy fold bit for bit;
  * ragged point counts with real guard rows behind the output; freshness of the folded stream (trainable: every call; frozen: invalidate_packed());
  * eval, SAVE 1 and SAVE 2 variants give the same raw, bit for bit.
"""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import _lib, ops
from oracle import c_oracle as co
from oracle import torch_port as tp
from helpers import CFGS, close, ref_state, tag_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = os.path.join(HERE, "golden", "trained_scene.ckpt")
ATOL = RTOL = 5e-6          # the project's own band for this kernel against the oracle


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _params(sd, prefix):
    return {k[len(prefix) + 5:]: v.to(DEV) for k, v in sd.items() if k.startswith(prefix + ".mlp.")}


def _both(sd, prefix, mode, pts, dirs):
    """(unfolded raw, folded raw) of the point kernels for one net."""
    params = _params(sd, prefix)
    plain = ops.mlp_forward_points(ops.pack_mlp(params, mode), mode, T(pts), T(dirs))
    folded = ops.mlp_forward_points(ops.pack_mlp(params, mode, precision="fp32_fold"), mode, T(pts), T(dirs), fold=True)
    return plain, folded


def _fp64_rgb(sd, prefix, cfg, pts, dirs):
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith(prefix + ".")}
    return tp.point_query(sd64, prefix, torch.as_tensor(pts).double(), torch.as_tensor(dirs).double(), cfg)[:, :3].numpy()


def _check_pair(sd, prefix, name, pts, dirs, what):
    mode = ops.sem_mode_of(**CFGS[name])
    plain, folded = _both(sd, prefix, mode, pts, dirs)
    ref = co.mlp(co.Weights(sd, prefix, **CFGS[name]), pts, dirs)
    truth = _fp64_rgb(sd, prefix, tp.PortConfig(**CFGS[name]), pts, dirs)
    e_plain = float(np.abs(N(plain)[:, :3] - truth).max())
    e_fold = float(np.abs(N(folded)[:, :3] - truth).max())
    d = float((folded[:, :3] - plain[:, :3]).abs().max())
    d_ref = float(np.abs(N(folded)[:, :3] - ref[:, :3]).max())
    print(f"view-fold {what}: max|rgb| {float(np.abs(truth).max()):.3g}  unfolded vs fp64 {e_plain:.3e}  folded vs fp64 {e_fold:.3e}  "
          f"folded vs unfolded {d:.3e}  folded vs oracle {d_ref:.3e}")
    assert torch.equal(folded[:, 3:], plain[:, 3:]), f"{what}: sigma / semantics must not move"
    close(N(folded)[:, :3], ref[:, :3], atol=ATOL, rtol=RTOL, what=f"{what}: folded rgb vs oracle")


# ------------------------------------------------------------------------------------------ folded against unfolded
@pytest.mark.parametrize("name", list(CFGS))
@pytest.mark.parametrize("peaky", [False, True])
def test_fold_vs_unfolded_golden_points(golden, manifest, name, peaky):
    g = golden("mlp")
    sd = ref_state(name, manifest, peaky)
    for prefix in ("nerf", "nerf_fine"):
        _check_pair(sd, prefix, name, g["pts"], g["dirs"], f"{tag_of(name, peaky)} {prefix}")


def test_fold_vs_unfolded_trained_field(golden):
    g = golden("trained")
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True)
    nerf_sos_amd.io.load_checkpoint(CKPT, net)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    rays = T(g["rays"])
    o, d = rays[0].reshape(-1, 3)[:96].contiguous(), rays[1].reshape(-1, 3)[:96].contiguous()
    near, far = (float(v) for v in g["near_far"])
    R = o.shape[0]
    z, v = ops.ray_setup(d, torch.full((R,), near, device=DEV), torch.full((R,), far, device=DEV), 64, None)
    pts = N(ops.ray_points(o, d, z)).reshape(-1, 3)
    dirs = N(v[:, None, :].expand(R, 64, 3)).reshape(-1, 3)
    for prefix in ("nerf", "nerf_fine"):
        _check_pair(sd, prefix, "semcoord", pts, dirs, f"trained_scene.ckpt {prefix}")


# ------------------------------------------------------------------------------------------ bitwise chain
_fmaf = None


def fmaf(a, b, c):
    """IEEE fp32 fused multiply-add (one rounding), the operation of the fp32 MFMA and of the oracle's chains."""
    global _fmaf
    if _fmaf is None:
        _fmaf = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").fmaf
        _fmaf.restype, _fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return np.float32(_fmaf(float(a), float(b), float(c)))


def numpy_fold(sd, prefix):
    """W' [128,256], b' [128]: fp64, j = 0..255 in order, multiply then add, ONE rounding to fp32."""
    Wv = sd[f"{prefix}.mlp.views_linears.0.weight"].numpy().astype(np.float64)
    bv = sd[f"{prefix}.mlp.views_linears.0.bias"].numpy().astype(np.float64)
    Wf = sd[f"{prefix}.mlp.feature_linear.weight"].numpy().astype(np.float64)
    bf = sd[f"{prefix}.mlp.feature_linear.bias"].numpy().astype(np.float64)
    acc, accb = np.zeros((128, 256)), np.zeros(128)
    for j in range(256):
        prod = Wv[:, j:j + 1] * Wf[j:j + 1, :]
        acc = acc + prod
        prodb = Wv[:, j] * bf[j]
        accb = accb + prodb
    accb = accb + bv
    return acc.astype(np.float32), accb.astype(np.float32)


def chain_feature(j):       # oracle/nerf_oracle.c: the k order of a hidden vector (0,4,1,5,2,6,3,7 per 8 features)
    q = j & 7
    return (j & ~7) + (q >> 1) + 4 * (q & 1)


@pytest.mark.parametrize("name", list(CFGS))
def test_fold_exact_chain_at_origin(manifest, name):
    sd = ref_state(name, manifest, peaky=True)
    mode = ops.sem_mode_of(**CFGS[name])
    prefix = "nerf_fine"
    pts = np.zeros((130, 3), np.float32)
    packed = ops.pack_mlp(_params(sd, prefix), mode, precision="fp32_fold")
    raw = N(ops.mlp_forward_points(packed, mode, T(pts), T(pts), fold=True))
    Wp, bp = numpy_fold(sd, prefix)
    # the fold as the device wrote it: [W' | W_v[:, 256:]] [128,283] and b' behind the chunks
    off = ops.packed_bytes(mode) // 4
    scratch = N(packed)[off:off + 128 * 283 + 128]
    Wv = sd[f"{prefix}.mlp.views_linears.0.weight"].numpy()
    assert np.array_equal(scratch[:128 * 283].reshape(128, 283)[:, :256], Wp), "W' in the packed buffer vs the numpy fold"
    assert np.array_equal(scratch[:128 * 283].reshape(128, 283)[:, 256:], Wv[:, 256:])
    assert np.array_equal(scratch[128 * 283:], bp), "b' in the packed buffer vs the numpy fold"
    # the oracle's own trunk (bitwise the kernel's at the origin: test_mlp_exact_fp32_chain) gives h7 and the unfolded raw
    ref, taps = co.mlp(co.Weights(sd, prefix, **CFGS[name]), pts[:1], pts[:1], taps=True)
    h7 = taps["h7"][0]
    ed = N(tp.posenc(torch.zeros(1, 3), 4))[0]                # 0 / 1 exactly
    assert set(np.unique(ed)) <= {0.0, 1.0}
    v = np.zeros(128, np.float32)
    for o in range(128):
        acc = bp[o]
        for j in range(256):
            f = chain_feature(j)
            acc = fmaf(Wp[o, f], h7[f], acc)
        for k in range(27):
            acc = fmaf(Wv[o, 256 + k], ed[k], acc)
        v[o] = max(acc, np.float32(0.0))
    rgb_w = sd[f"{prefix}.mlp.rgb_linear.weight"].numpy()
    rgb_b = sd[f"{prefix}.mlp.rgb_linear.bias"].numpy()
    want = ref[0].copy()
    for c in range(3):                                        # dot_halves
        lo, hi = np.float32(rgb_b[c]), np.float32(0.0)
        for f in range(128):
            if f & 4:
                hi = fmaf(rgb_w[c, f], v[f], hi)
            else:
                lo = fmaf(rgb_w[c, f], v[f], lo)
        want[c] = np.float32(lo + hi)
    assert np.array_equal(raw, np.broadcast_to(want, raw.shape)), f"max abs diff {np.abs(raw - want).max():.3e}"


# ------------------------------------------------------------------------------------------ ragged point counts
@pytest.mark.parametrize("n_pts", [1, 31, 129, 128 * 300 + 5])
def test_fold_ragged_point_counts(manifest, n_pts):
    sd = ref_state("semcoord", manifest, peaky=True)
    rng = np.random.default_rng(n_pts)
    pts = (rng.random((n_pts, 3), dtype=np.float32) * 8 - 4)
    dirs = rng.standard_normal((n_pts, 3), dtype=np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    params = _params(sd, "nerf_fine")
    plain = ops.mlp_forward_points(ops.pack_mlp(params, 2), 2, T(pts), T(dirs))
    packed = ops.pack_mlp(params, 2, precision="fp32_fold")
    raw = ops.mlp_forward_points(packed, 2, T(pts), T(dirs), fold=True)
    assert raw.shape == (n_pts, 6)
    assert torch.equal(raw[:, 3:], plain[:, 3:])
    sel = np.unique(np.concatenate([np.arange(min(n_pts, 40)), np.arange(max(0, n_pts - 40), n_pts), rng.integers(0, n_pts, 40)]))
    ref = co.mlp(co.Weights(sd, "nerf_fine", True, True), pts[sel], dirs[sel])
    print(f"view-fold ragged n_pts={n_pts}: folded vs unfolded {float((raw[:, :3] - plain[:, :3]).abs().max()):.3e}  "
          f"folded vs oracle {float(np.abs(N(raw)[sel, :3] - ref[:, :3]).max()):.3e}")
    close(N(raw)[sel, :3], ref[:, :3], atol=ATOL, rtol=RTOL, what=f"n_pts={n_pts}: folded rgb vs oracle")
    # every row, interior tiles included: both kernels are granted 5e-6 + 5e-6 |ref| against the oracle, so they lie within twice that of
    # each other
    close(N(raw)[:, :3], N(plain)[:, :3], atol=2 * ATOL, rtol=2 * RTOL, what=f"n_pts={n_pts}: folded rgb vs unfolded, all rows")
    # guard rows: the folded entry points write into an output that is 64 rows longer than the batch; those rows must stay untouched
    L, P = _lib.lib(), (lambda t: ctypes.c_void_p(t.data_ptr()))
    p_d, d_d = T(pts), T(dirs)
    out = torch.full((n_pts + 64, 6), 777.0, device=DEV)
    _lib.check(L.nsos_mlp_forward_points_fold(P(packed), 2, P(p_d), P(d_d), n_pts, P(out), None), "nsos_mlp_forward_points_fold")
    torch.cuda.synchronize()
    assert torch.equal(out[:n_pts], raw) and bool((out[n_pts:] == 777.0).all()), "points entry wrote past n_pts"
    zero3, zero1 = torch.zeros_like(p_d), torch.zeros((n_pts, 1), device=DEV)      # rays of one sample: o + 0 * 0 is the point, bit for bit
    out = torch.full((n_pts + 64, 6), 777.0, device=DEV)
    _lib.check(L.nsos_mlp_forward_rays_fold(P(packed), 2, P(p_d), P(zero3), P(d_d), P(zero1), n_pts, 1, P(out), None), "nsos_mlp_forward_rays_fold")
    torch.cuda.synchronize()
    assert torch.equal(out[:n_pts], raw) and bool((out[n_pts:] == 777.0).all()), "rays entry wrote past n_pts"
    # the two streams are told apart by their size: each kernel family refuses the other's buffer
    with pytest.raises(ValueError, match="fp32_fold"):
        ops.mlp_forward_points(ops.pack_mlp(params, 2), 2, T(pts), T(dirs), fold=True)
    with pytest.raises(ValueError, match="fold=True"):
        ops.mlp_forward_points(packed, 2, T(pts), T(dirs))


# ------------------------------------------------------------------------------------------ freshness
def _render(net, rays):
    with torch.no_grad():
        out = net(rays, (tp.NEAR, tp.FAR), radii=None)
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("frozen", [False, True])
def test_fold_follows_data_edits(manifest, frozen):
    """feature_linear.weight and views_linears.0.bias both enter the fold: `.data` edits (no version bump, what fused Adam does)
    must reach the next forward of a trainable net, and that of a frozen net after invalidate_packed()."""
    sd = ref_state("semcoord", manifest)
    rays = T(tp.synthetic_rays(64, seed=5))

    def make():
        net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS["semcoord"]).to(DEV).eval()
        net.load_state_dict(sd)
        for p in net.parameters():
            p.requires_grad_(not frozen)
        return net

    net = make()
    before = _render(net, rays)
    edited = {k: v.clone() for k, v in sd.items()}
    gen = torch.Generator().manual_seed(1)
    for pre, m in (("nerf", net.nerf), ("nerf_fine", net.nerf_fine)):
        dw = 0.05 * torch.randn(256, 256, generator=gen)
        db = 0.05 * torch.randn(128, generator=gen)
        edited[f"{pre}.mlp.feature_linear.weight"] += dw
        edited[f"{pre}.mlp.views_linears.0.bias"] += db
        versions = (m.mlp.feature_linear.weight._version, m.mlp.views_linears[0].bias._version)
        m.mlp.feature_linear.weight.data.add_(dw.to(DEV))
        m.mlp.views_linears[0].bias.data.add_(db.to(DEV))
        assert versions == (m.mlp.feature_linear.weight._version, m.mlp.views_linears[0].bias._version)
    if frozen:
        net.invalidate_packed()
    after = _render(net, rays)
    fresh = make()
    fresh.load_state_dict(edited)
    want = _render(fresh, rays)
    assert not torch.equal(after["rgb"], before["rgb"])
    for k in want:
        assert torch.equal(after[k], want[k]), k


# ------------------------------------------------------------------------------------------ variants
@pytest.mark.parametrize("name", list(CFGS))
def test_fold_variants_agree_bitwise(manifest, name):
    sd = ref_state(name, manifest, peaky=True)
    mode = ops.sem_mode_of(**CFGS[name])
    R = 300
    rays = T(tp.synthetic_rays(R, seed=2))
    o, d = rays[0].contiguous(), rays[1].contiguous()
    z, v = ops.ray_setup(d, torch.full((R,), tp.NEAR, device=DEV), torch.full((R,), tp.FAR, device=DEV), 64, None)
    params = _params(sd, "nerf_fine")
    packed = ops.pack_mlp(params, mode, precision="fp32_fold")
    raw = ops.mlp_forward_rays(packed, mode, o, d, v, z, fold=True)
    plain = ops.mlp_forward_rays(ops.pack_mlp(params, mode), mode, o, d, v, z)
    assert torch.equal(raw[..., 3:], plain[..., 3:])
    raw2, acts, _ = ops.mlp_forward_rays_save_all(packed, mode, o, d, v, z, fold=True)
    assert torch.equal(raw2, raw), "SAVE 2 raw"
    _, acts_plain, _ = ops.mlp_forward_rays_save_all(ops.pack_mlp(params, mode), mode, o, d, v, z)
    A = ops.ACTS_VIEWS
    assert torch.equal(acts[:, :A], acts_plain[:, :A]), "trunk activations and the feature vector are the unfolded kernel's"
    if mode != ops.SEM_NONE:     # (without a semantic head nobody writes the NSOS_ACTS_SEM block: uninitialised memory in both)
        assert torch.equal(acts[:, ops.ACTS_SEM:ops.ACTS_X], acts_plain[:, ops.ACTS_SEM:ops.ACTS_X])
    assert torch.equal(acts[:, ops.ACTS_X:], acts_plain[:, ops.ACTS_X:])
    # the saved view-layer activations come from the folded chain: they move by rounding, and stay far inside the 1e-4 bar the
    # gradients formed from them are held to (tests/test_gpu_backward*.py)
    dv = float((acts[:, A:A + 128] - acts_plain[:, A:A + 128]).abs().max())
    print(f"view-fold {name}: saved view activations, folded vs unfolded {dv:.3e} (max |v| {float(acts_plain[:, A:A + 128].abs().max()):.3g})")
    close(N(acts[:, A:A + 128]), N(acts_plain[:, A:A + 128]), atol=1e-4, rtol=1e-4, what="saved view activations")
    if mode != ops.SEM_NONE:
        raw1, sem_in, sem_hid = ops.mlp_forward_rays_save(packed, mode, o, d, v, z, fold=True)
        assert torch.equal(raw1, raw), "SAVE 1 raw"
        _, sem_in_p, sem_hid_p = ops.mlp_forward_rays_save(ops.pack_mlp(params, mode), mode, o, d, v, z)
        assert torch.equal(sem_in, sem_in_p) and torch.equal(sem_hid, sem_hid_p)
