"""GPU: the small kernels between the MLP and the loss, each alone against its fp64 reference (tests/render_tail_port.py, validated on
the CPU by tests/test_render_tail_port.py).

composite_backward_kernel<IPL, NS> -- S at both edges of every IPL template (1, 2, 3, 4, 8), C = 4, 5, 6 (NS = 2) and 7, 9, 12
(NS = 8), white / black background, sigma noise or none, a dense and a thin sigma regime (in the thin one acc stays inside (0, 1), so
G_acc and the disp terms do not cancel), all six upstream gradients together and each one alone (the others NULL).  Per element
    |got - want| <= K 2^-24 M(ray, column group),       exactly 0 where M = 0,
with M the largest magnitude (every summed product taken absolute) over the ray's samples and the columns of the group (colour,
sigma, semantics).  K = 4 x 188.31 = 753.24: the reference's own fp32 autograd is up to 188.31 units away from fp64 on this case
list (CPU test); the factor 4 covers the kernel's correctly rounded exp against libm's and its different association.
Measured on the MI355X: the kernel's worst ratio is 187.2 units (S = 512, thin, upstream weights; 155.1 at S = 300, at most 123 up to
S = 257) -- about the fp32 reference's own distance: both round alpha = 1 - exp(-sigma dist) to fp32 before t = 1 - alpha.

ray_grad_reduce_kernel -- alone, R = 1, 7, 37, S around the 64-lane stride, C = 4, 6, 12, |d| x 0.01, 1, 30, rows with sigma <= 0
throughout, with / without g_dirs and noise; g_pts only, g_dirs only, g_raw only (with and without noise) and all together, so every
term is held at its own scale:  |got - want| <= 8 2^-24 Y  (derived, not measured: every summed term carries at most three fp32
roundings -- noise * std, the add, the product --, the sums and the tail are fp64, the result is rounded once; the factor 2 is
slack).  Measured: 2.22 units at worst (S = 1, g_raw with noise); at most 0.53 where no noise enters.

render_draws_kernel -- bit for bit: the uniforms equal the port's Philox4x32-10 stream exactly (tensor offsets with sizes that are
no multiple of 4, absent tensors, the high key word, the high call word, the device-resident call counter), and lie strictly inside
(0, 1) also where the word is all ones in its top bits.  The normals are finite and within 2^-10 absolute of the fp64 Box-Muller of
the same words: an identity check (a mixed-up word moves a normal by O(1)), not an accuracy claim -- the fast __logf / __sinf /
__cosf intrinsics have no citable error bound.  Measured: at most 1.6e-6 over every case here.  The high word of the block index (counter word 1)
needs more than 2^32 blocks in one call and stays untested.
"""
import numpy as np
import pytest
import torch

from nerf_sos_amd import ops
from oracle import torch_port as tp
import render_tail_port as rtp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------ compositing backward
@pytest.mark.parametrize("S", rtp.COMPOSITE_S)
def test_composite_backward_vs_fp64_closed_form(S):
    worst = (0.0, None)
    for C, regime, white, noisy in rtp.composite_configs(S):
        case = rtp.composite_case(S, C, regime, white, noisy)
        args = (case["raw"], case["z"], case["d"], case["noise"], case["std"], white)
        dev = [T(a) for a in args[:4]]
        for name, ups in rtp.upstream_sets(case["ups"]):
            want = rtp.composite_backward_closed(*args, ups)
            M = rtp.group_scale(rtp.composite_backward_closed(*args, ups, absolute=True))
            got = ops.composite_backward(*dev, case["std"], white, g_rgb=T(ups.get("rgb")), g_sem=T(ups.get("semantics")),
                                         g_depth=T(ups.get("depth")), g_acc=T(ups.get("acc")), g_disp=T(ups.get("disp")),
                                         g_weights=T(ups.get("weights"))).cpu().double()
            what = f"S={S} C={C} {regime} white={white} noisy={noisy} upstream={name}"
            assert torch.isfinite(got).all(), what
            assert (got[M == 0] == 0).all(), f"{what}: a gradient where nothing is summed"
            ratio = torch.where(M > 0, (got - want).abs() / torch.where(M > 0, M * rtp.U24, torch.ones_like(M)), torch.zeros_like(M))
            r = float(ratio.max())
            if r > worst[0]:
                worst = (r, what)
            assert r <= rtp.COMPOSITE_K, f"{what}: {r:.1f} units of 2^-24 M at {np.unravel_index(int(ratio.argmax()), ratio.shape)} (K = {rtp.COMPOSITE_K})"
    print(f"composite_backward S={S}: worst {worst[0]:.2f} units ({worst[1]}); K = {rtp.COMPOSITE_K}")


# ------------------------------------------------------------------------------------------ compositing forward, the remaining widths
@pytest.mark.parametrize("C", [5, 7, 9, 12])
@pytest.mark.parametrize("S", [64, 100, 192])
def test_composite_forward_other_channel_counts(C, S):
    """ops.composite at C = 5 and through the two-semantic-channels-per-launch path (C > 6) against the fp64 port, at the bounds
    test_composite holds against the reference."""
    from helpers import close
    g = torch.Generator().manual_seed(S * 100 + C)
    R = 37
    noisy, white = bool(C & 1), bool((C + S // 64) & 2)
    raw = torch.randn(R, S, C, generator=g) * 2
    z = torch.sort(1.2 + 13 * torch.rand(R, S, generator=g), -1)[0]
    d = torch.randn(R, 3, generator=g)
    noise = torch.randn(R, S, generator=g) if noisy else None
    out = ops.composite(T(raw), T(z), T(d), T(noise), 0.75 if noisy else 0.0, white)
    ref = tp.composite(raw.double(), z.double(), d.double(), noise.double() * 0.75 if noisy else None,
                       tp.PortConfig(use_semantics=True, white_bkgd=white))
    assert set(out) == set(ref) and out["semantics"].shape == (R, C - 4)
    for k in ref:
        close(out[k].cpu().numpy(), ref[k].numpy(), atol=2e-6, rtol=2e-5, what=f"C={C} S={S} {k} vs fp64 port")


# ------------------------------------------------------------------------------------------ ray-gradient reduce
@pytest.mark.parametrize("S", rtp.RAYGRAD_S)
def test_ray_grad_reduce_vs_fp64_closed_form(S):
    worst = (0.0, None)
    i = 0
    for R in rtp.RAYGRAD_R:
        for C in rtp.RAYGRAD_C:
            for scale in rtp.RAYGRAD_SCALE:
                i += 1
                case = rtp.raygrad_case(R, S, C, scale, seed=1000 * S + i)
                std = (0.5, 0.75)[i & 1]
                rot_noise = case["noise"] if i & 2 else None
                rot_dirs = case["g_dirs"] if i % 3 else None
                zero_pts, zero_raw = torch.zeros_like(case["g_pts"]), torch.zeros_like(case["g_raw"])
                sets = {"g_pts": (case["g_pts"], None, zero_raw, rot_noise), "g_dirs": (zero_pts, case["g_dirs"], zero_raw, rot_noise),
                        "g_raw": (zero_pts, None, case["g_raw"], None), "g_raw+noise": (zero_pts, None, case["g_raw"], case["noise"]),
                        "all": (case["g_pts"], rot_dirs, case["g_raw"], rot_noise)}
                for name, (g_pts, g_dirs, g_raw, noise) in sets.items():
                    g_o, g_d = ops.ray_grad_reduce(T(g_pts), T(g_dirs), T(case["z"]), T(case["d"]), T(case["raw"]), T(g_raw), T(noise), std)
                    w_o, w_d, Y_o, Y_d = rtp.ray_grad_reduce_closed(g_pts, g_dirs, case["z"], case["d"], case["raw"], g_raw, noise, std)
                    what = f"S={S} R={R} C={C} |d|x{scale} std={std} {name} dirs={g_dirs is not None} noise={noise is not None}"
                    g_o, g_d = g_o.cpu().double(), g_d.cpu().double()
                    assert g_o.shape == (R, 3) and g_d.shape == (R, 3) and torch.isfinite(g_o).all() and torch.isfinite(g_d).all(), what
                    if name in ("g_dirs", "g_raw", "g_raw+noise"):
                        assert (g_o == 0).all(), f"{what}: g_o must be exactly 0"
                    else:
                        assert float(w_o.abs().max()) > 0
                    assert float(w_d.abs().max()) > 0 or (name.startswith("g_raw") and (R == 1 or S == 1)), what
                    for got, want, Y, which in ((g_o, w_o, Y_o, "g_o"), (g_d, w_d, Y_d, "g_d")):
                        err = (got - want).abs()
                        r = float(torch.where(Y > 0, err / torch.where(Y > 0, Y * rtp.U24, torch.ones_like(Y)), torch.zeros_like(Y)).max())
                        if r > worst[0]:
                            worst = (r, f"{what} {which}")
                        assert (err <= 8 * rtp.U24 * Y).all(), f"{what}: {which} off by {r:.2f} units of 2^-24 Y (bound 8)"
    print(f"ray_grad_reduce S={S}: worst {worst[0]:.3f} units ({worst[1]}); bound 8")


# ------------------------------------------------------------------------------------------ the Philox draws
NORMAL_BOUND = 2.0 ** -10


def _check_draws(got, want, what):
    """Uniforms equal the port exactly and lie strictly inside (0, 1); normals are finite and within NORMAL_BOUND.  Returns the largest
    deviation of a normal."""
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        name = ("t_rand", "noise0", "u", "noise1")[i]
        assert (g is None) == (w is None), f"{what}: {name} present / absent"
        if g is None:
            continue
        g = g.cpu()
        assert g.dtype == torch.float32 and g.shape == w.shape, f"{what}: {name}"
        if i in (0, 2):
            assert float(g.min()) > 0.0 and float(g.max()) < 1.0, f"{what}: {name} leaves (0, 1): [{float(g.min())!r}, {float(g.max())!r}]"
            assert torch.equal(w.float().double(), w), "the documented uniforms are fp32 numbers"
            assert torch.equal(g, w.float()), f"{what}: {name} differs from the port in {int((g != w.float()).sum())} of {g.numel()} elements"
        else:
            assert torch.isfinite(g).all(), f"{what}: {name} not finite"
            dev = float((g.double() - w).abs().max())
            worst = max(worst, dev)
            assert dev <= NORMAL_BOUND, f"{what}: {name} is {dev:.3e} from the fp64 Box-Muller of its words"
    return worst


SEEDS = (1234, 0x9E3779B97F4A7C15)      # the second uses the high key word
CALLS = (1, 2 ** 32 + 5)                # the second uses the high counter word


@pytest.mark.parametrize("R,S,N", [(5, 3, 0), (33, 7, 5), (7, 64, 128), (257, 64, 128)])
def test_render_draws_equal_the_philox_port(R, S, N):
    worst = 0.0
    for seed in SEEDS:
        for call in CALLS:
            got = ops.render_draws(seed, call, R, S, N, DEV)
            worst = max(worst, _check_draws(got, rtp.render_draws_port(seed, call, R, S, N), f"seed={seed:#x} call={call} R={R} S={S} N={N}"))
    print(f"render_draws R={R} S={S} N={N}: normals within {worst:.3e} of fp64 Box-Muller (bound {NORMAL_BOUND:.3e})")


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("importance", [False, True])
def test_render_draws_absent_tensors_shift_the_offsets(jitter, noise, importance):
    R, S, N = 33, 7, 5                  # 231, 231, 165, 396 elements: none a multiple of 4
    for seed, call in zip(SEEDS, CALLS):
        got = ops.render_draws(seed, call, R, S, N, DEV, jitter=jitter, noise=noise, importance=importance)
        _check_draws(got, rtp.render_draws_port(seed, call, R, S, N, jitter, noise, importance), f"jitter={jitter} noise={noise} importance={importance}")


@pytest.mark.parametrize("k", [41, 2 ** 32 + 4])
def test_render_draws_device_counter(k):
    """`call` as an int64 device tensor holding k draws the values of call = k + 1 and leaves k + 1 in the tensor."""
    R, S, N = 33, 7, 5
    counter = torch.tensor([k], dtype=torch.int64, device=DEV)
    got = ops.render_draws(SEEDS[1], counter, R, S, N, DEV)
    _check_draws(got, rtp.render_draws_port(SEEDS[1], k + 1, R, S, N), f"device counter {k}")
    assert int(counter.item()) == k + 1
    again = ops.render_draws(SEEDS[1], counter, R, S, N, DEV)
    _check_draws(again, rtp.render_draws_port(SEEDS[1], k + 2, R, S, N), f"device counter {k + 1}")
    assert int(counter.item()) == k + 2


@pytest.mark.parametrize("edge", sorted(rtp.EDGE_CALLS))
def test_render_draws_edge_words(edge):
    """Calls (found with the port, tests/render_tail_port.find_edge_calls) in which a word >= 0xFFFFFF00 or < 0x100 lands in t_rand,
    or a word >= 0xFFFFFF00 in a normal's u0 slot: the uniforms stay strictly inside (0, 1) -- (k + 0.5) 2^-24 in fp32 gave exactly
    1.0 for the first -- and the normals finite (ln u0 stays negative)."""
    R, S, call = rtp.EDGE_R, rtp.EDGE_S, rtp.EDGE_CALLS[edge]
    words = rtp.render_draws_words(rtp.EDGE_SEED, call, R, S, 0)
    hit = {"t_rand_high": words[0] >= 0xFFFFFF00, "t_rand_low": words[0] < 0x100, "normal_u0_high": words[1][0::2] >= 0xFFFFFF00}[edge]
    assert hit.any(), "the committed call number does not hold its edge word"
    got = ops.render_draws(rtp.EDGE_SEED, call, R, S, 0, DEV)
    worst = _check_draws(got, rtp.render_draws_port(rtp.EDGE_SEED, call, R, S, 0), f"{edge} call={call}")
    print(f"render_draws {edge} (call {call}): normals within {worst:.3e}")
