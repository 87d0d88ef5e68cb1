"""CPU: the fp64 references of tests/render_tail_port.py are themselves right, and their bounds mean something.

* Philox4x32-10 reproduces the published known answers; the committed edge calls hold the edge words they were searched for; the
  23-bit uniform is exact in fp32 for every word and stays inside (0, 1), which the 24-bit (k + 0.5) 2^-24 did not.
* The signed closed form of the compositing backward equals fp64 autograd through oracle/torch_port.composite on every case of
  tests/test_gpu_render_tail.py, each upstream gradient alone and all together (measured: <= 9e-8 units).
* The reference's own fp32 autograd (the same port in float32) is at most 256 units of 2^-24 M away from fp64 over that case
  list (measured: 188.3, at S = 512 thin; 128 of the 156 configurations stay below 50) -- the GPU test allows the kernel 4 x that.
* Each upstream gradient alone reaches >= 1e5 units somewhere in the thin regime (measured: >= 9.7e6 for all six, g_acc
  included): a kernel that dropped one would be caught.
* The ray-gradient closed form equals fp64 autograd of pts = o + d z, v = d / |d| and the compositing's dists * |d|.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
import render_tail_port as rtp

KNOWN_ANSWERS = [      # Random123's kat_vectors for philox4x32 10
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_philox_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        assert " ".join(f"{int(x):08x}" for x in rtp.philox4x32_10(ctr, key)) == want
    ctrs = np.array([k[0] for k in KNOWN_ANSWERS], dtype=np.uint64)          # vectorised over counters and keys at once
    keys = np.array([k[1] for k in KNOWN_ANSWERS], dtype=np.uint64)
    got = rtp.philox4x32_10(ctrs, keys)
    assert [" ".join(f"{int(x):08x}" for x in row) for row in got] == [k[2] for k in KNOWN_ANSWERS]


def test_uniform_formula_is_exact_in_fp32_and_open():
    """(k + 0.5) 2^-23 over the top 23 bits, evaluated in fp32 as the kernel does, equals the fp64 value for all 2^23 k and stays
    inside (0, 1); the 24-bit (k + 0.5) 2^-24 ties for every k >= 2^23 and gives exactly 1.0 at k = 2^24 - 1."""
    k = np.arange(1 << 23, dtype=np.uint32)
    f32 = (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert f32.dtype == np.float32
    want = rtp.uniform_from_word(k.astype(np.uint64) << np.uint64(9))
    assert np.array_equal(f32.astype(np.float64), want)
    assert want.min() == 2.0 ** -24 and want.max() == 1.0 - 2.0 ** -24
    old = (np.float32(2 ** 24 - 1) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert old == np.float32(1.0)


def test_edge_calls_hold_their_words():
    R, S = rtp.EDGE_R, rtp.EDGE_S
    w = {k: rtp.render_draws_words(rtp.EDGE_SEED, c, R, S, 0) for k, c in rtp.EDGE_CALLS.items()}
    assert (w["t_rand_high"][0] >= 0xFFFFFF00).any()
    assert (w["t_rand_low"][0] < 0x100).any()
    assert (w["normal_u0_high"][1][0::2] >= 0xFFFFFF00).any()
    for k, c in rtp.EDGE_CALLS.items():
        t, n0, u, n1 = rtp.render_draws_port(rtp.EDGE_SEED, c, R, S, 0)
        assert u is None and n1 is None and t.shape == (R, S) and n0.shape == (R, S)
        assert 0.0 < float(t.min()) and float(t.max()) < 1.0 and torch.equal(t.float().double(), t)
        assert torch.isfinite(n0).all()


def test_draws_layout():
    """Absent tensors take no blocks (the offsets of the later ones shift); a tensor's values do not depend on its own tail."""
    full = rtp.render_draws_words(7, 3, 33, 7, 5)
    assert [w.size for w in full] == [231, 231, 165, 396]
    no_jitter = rtp.render_draws_words(7, 3, 33, 7, 5, jitter=False)
    assert no_jitter[0] is None and np.array_equal(no_jitter[1][:228], full[0][:228])     # noise0 now starts at block 0
    assert np.array_equal(rtp.render_draws_words(7, 3, 33, 7, 0)[0], full[0])
    hi = rtp.render_draws_words(7, 2 ** 32 + 3, 33, 7, 5)
    assert not np.array_equal(hi[0], full[0])                                             # the high counter word counts


# ------------------------------------------------------------------------------------------ compositing backward
def _autograd(case, ups, dtype):
    raw = case["raw"].to(dtype).detach().clone().requires_grad_(True)
    nz = None if case["noise"] is None else case["noise"].to(dtype) * case["std"]
    cfg = tp.PortConfig(use_semantics=raw.shape[-1] > 4, white_bkgd=case["white"])
    ret = tp.composite(raw, case["z"].to(dtype), case["d"].to(dtype), nz, cfg)
    sum((ret[k] * ups[k].to(dtype).reshape(ret[k].shape)).sum() for k in ups).backward()
    return raw.grad.double(), ret["acc"].detach().double()


@functools.lru_cache(maxsize=None)
def _measure(S):
    """Per (configuration, upstream set) at S samples: the closed form's distance from fp64 autograd, the fp32 autograd's distance
    from fp64, and the size of the fp64 gradient -- all in units of 2^-24 M."""
    rows = []
    for C, regime, white, noisy in rtp.composite_configs(S):
        case = rtp.composite_case(S, C, regime, white, noisy)
        args = (case["raw"], case["z"], case["d"], case["noise"], case["std"], white)
        for name, ups in rtp.upstream_sets(case["ups"]):
            want, acc = _autograd(case, ups, torch.float64)
            ref32, _ = _autograd(case, ups, torch.float32)
            got = rtp.composite_backward_closed(*args, ups)
            M = rtp.group_scale(rtp.composite_backward_closed(*args, ups, absolute=True))
            assert torch.isfinite(want).all() and torch.isfinite(got).all() and torch.isfinite(ref32).all()
            assert ((M > 0) | ((want == 0) & (got == 0) & (ref32 == 0))).all(), "no magnitude, no gradient"
            unit = torch.where(M > 0, M * rtp.U24, torch.ones_like(M))
            rows.append(dict(C=C, regime=regime, white=white, noisy=noisy, ups=name, closed=float(((got - want).abs() / unit).max()),
                             ref32=float(((ref32 - want).abs() / unit).max()), size=float((want.abs() / unit).max()),
                             acc_median=float(acc.median())))
    return rows


@pytest.mark.parametrize("S", rtp.COMPOSITE_S)
def test_composite_backward_closed_form_equals_fp64_autograd(S):
    """Bound 1e-4 units: both sides are fp64 (2^-53 per operation) over at most ~4 x 512 summed terms, ~4e-6 units; measured 9e-8."""
    rows = _measure(S)
    assert {r["ups"] for r in rows} == {"all", *rtp.UPSTREAMS}
    worst = max(rows, key=lambda r: r["closed"])
    print(f"S={S}: closed form vs fp64 autograd, worst {worst['closed']:.2e} units ({worst})")
    assert worst["closed"] <= 1e-4, worst


def test_composite_backward_fp32_reference_stays_within_256_units():
    rows = [dict(r, S=S) for S in rtp.COMPOSITE_S for r in _measure(S)]
    worst = max(rows, key=lambda r: r["ref32"])
    per_config = {}
    for r in rows:
        key = (r["S"], r["C"], r["regime"])
        per_config[key] = max(per_config.get(key, 0.0), r["ref32"])
    print(f"fp32 autograd vs fp64: worst {worst['ref32']:.2f} units ({worst}); "
          f"{sum(v <= 50 for v in per_config.values())} of {len(per_config)} configurations <= 50 units")
    assert worst["ref32"] <= 256, worst
    assert rtp.COMPOSITE_K == 4 * rtp.REF_WORST <= 4 * 256          # the GPU test's K: 4 x the figure recorded from this measurement


def test_composite_backward_every_upstream_is_visible_in_the_thin_regime():
    rows = [r for S in rtp.COMPOSITE_S for r in _measure(S) if r["regime"] == "thin"]
    accs = sorted(r["acc_median"] for S in rtp.COMPOSITE_S if S >= 63 for r in _measure(S) if r["regime"] == "thin" and r["ups"] == "all")
    print(f"thin regime, S >= 63: median acc per configuration from {accs[0]:.3f} to {accs[-1]:.3f}")
    assert 0.2 <= accs[0] and accs[-1] <= 0.98, "the thin rays are neither empty nor opaque"
    for name in rtp.UPSTREAMS:
        size = max(r["size"] for r in rows if r["ups"] == name)
        print(f"upstream {name} alone: fp64 gradient reaches {size:.3g} units")
        assert size >= 1e5, name


# ------------------------------------------------------------------------------------------ ray-gradient reduce
@pytest.mark.parametrize("R,S,C,scale,with_dirs,noisy", [(7, 1, 4, 1.0, True, True), (7, 50, 6, 0.01, True, False), (5, 65, 12, 30.0, False, True),
                                                         (3, 192, 4, 1.0, True, True), (1, 64, 6, 30.0, False, False)])
def test_ray_grad_reduce_closed_form_equals_fp64_autograd(R, S, C, scale, with_dirs, noisy):
    """pts = o + d z, v = d / |d| and alpha(dists |d|) built in torch; g_raw[..., 3] and the |d| term both come from autograd.
    Bound 1e-4 units of 2^-24 Y (fp64 on both sides)."""
    case = rtp.raygrad_case(R, S, C, scale, seed=S * 10 + C)
    std = 0.75
    o = torch.zeros(R, 3, dtype=torch.float64, requires_grad=True)
    d = case["d"].double().requires_grad_(True)
    raw = case["raw"].double().requires_grad_(True)
    z = case["z"].double()
    noise = case["noise"] if noisy else None
    A, B = case["g_pts"].double().reshape(R, S, 3), case["g_dirs"].double().reshape(R, S, 3)
    Wt = torch.randn(R, S, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    v = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    ret = tp.composite(raw, z, d, None if noise is None else noise.double() * std, tp.PortConfig(use_semantics=C > 4))
    loss = (pts * A).sum() + (ret["weights"] * Wt).sum()
    if with_dirs:
        loss = loss + (v[:, None, :].expand(R, S, 3) * B).sum()
    loss.backward()
    g_o, g_d, Y_o, Y_d = rtp.ray_grad_reduce_closed(case["g_pts"], case["g_dirs"] if with_dirs else None, case["z"], case["d"], case["raw"],
                                                    raw.grad, noise, std)
    assert (S == 1 or R == 1 or float(raw.grad[..., 3].abs().max()) > 0) and (raw.grad[::3, :, 3] == 0).all(), "rows with sigma <= 0 throughout"
    assert ((g_o - o.grad).abs() <= 1e-4 * rtp.U24 * Y_o).all()
    assert ((g_d - d.grad).abs() <= 1e-4 * rtp.U24 * Y_d).all(), float(((g_d - d.grad).abs() / (rtp.U24 * Y_d)).max())
