"""TEST INFRASTRUCTURE -- plain fp64 references for the kernels between the MLP and the loss (numpy / torch, no GPU):

* ``philox4x32_10`` / ``render_draws_port``   <- render_draws_kernel (csrc/sampling.hip), written from the layout in its header comment
* ``composite_backward_closed``               <- the formulas in the comment above composite_backward_kernel (csrc/composite.hip)
* ``ray_grad_reduce_closed``                  <- the formulas in the comment above ray_grad_reduce_kernel (csrc/mlp_generic.hip)

The closed forms also return the MAGNITUDE of what they sum (every summed product replaced by its absolute value): the scale an
fp32 rounding error of a term is measured against.  tests/test_render_tail_port.py validates all of this on the CPU (published
Philox known answers, fp64 autograd through oracle/torch_port.composite); tests/test_gpu_render_tail.py holds the kernels to it.
The input generators of both files live here too, so the CPU validation and the GPU comparison run the same cases.
"""
import math

import numpy as np
import torch

U24 = 2.0 ** -24          # one unit of the bounds: half an fp32 ulp of 1

# ------------------------------------------------------------------------------------------ Philox4x32-10
_M0, _M1, _W0, _W1, _LO = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)


def philox4x32_10(counter4, key2):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11), vectorised: counter4 [..., 4] and key2 [..., 2] (broadcast against each
    other) of 32-bit words -> uint32 [..., 4]."""
    c = np.asarray(counter4, dtype=np.uint64)
    k = np.asarray(key2, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                           # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def draw_sizes(R, S, N, jitter=True, noise=True, importance=True):
    """Element counts of (t_rand [R,S], noise0 [R,S], u [R,N], noise1 [R,S+N]); 0 where the tensor is absent."""
    fine = N > 0
    return (R * S if jitter else 0, R * S if noise else 0, R * N if (importance and fine) else 0, R * (S + N) if (noise and fine) else 0)


def render_draws_blocks(seed, call, R, S, N, jitter=True, noise=True, importance=True):
    """The Philox blocks behind the four tensors, each uint32 [ceil(size / 4), 4] (None where absent): each present tensor is
    padded to a multiple of 4, the global block index b runs over the four tensors in order, block b is
    Philox(counter = (b_lo, b_hi, call_lo, call_hi), key = (seed_lo, seed_hi)) and element e is word e & 3 of block e >> 2."""
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    sizes = draw_sizes(R, S, N, jitter, noise, importance)
    quads = [(n + 3) // 4 for n in sizes]
    b = np.arange(sum(quads), dtype=np.uint64)
    ctr = np.stack([b & _LO, b >> _S32, np.full_like(b, call & 0xFFFFFFFF), np.full_like(b, call >> 32)], -1)
    words = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    out, b0 = [], 0
    for n, q in zip(sizes, quads):
        out.append(words[b0:b0 + q] if n else None)
        b0 += q
    return out


def render_draws_words(seed, call, R, S, N, jitter=True, noise=True, importance=True):
    """The 32-bit word behind every element of the four tensors: flat uint32 arrays of the tensors' sizes (None where absent)."""
    sizes = draw_sizes(R, S, N, jitter, noise, importance)
    return [None if b is None else b.reshape(-1)[:n] for b, n in zip(render_draws_blocks(seed, call, R, S, N, jitter, noise, importance), sizes)]


def uniform_from_word(x):
    """The documented uniform of a 32-bit word, in fp64: (k + 0.5) 2^-23 with k the word's top 23 bits -- inside
    [2^-24, 1 - 2^-24], every value an fp32 number."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals_from_words(x):
    """fp64 Box-Muller over a flat word array padded to whole blocks of 4: word pairs (0,1) and (2,3) of a block give
    (r cos t, r sin t) with r = sqrt(-2 ln u0), t = 2 pi u1."""
    u = uniform_from_word(x).reshape(-1, 2)
    r, th = np.sqrt(-2.0 * np.log(u[:, 0])), 2.0 * math.pi * u[:, 1]
    return np.stack([r * np.cos(th), r * np.sin(th)], -1).reshape(-1)


def render_draws_port(seed, call, R, S, N, jitter=True, noise=True, importance=True):
    """(t_rand [R,S], noise0 [R,S], u [R,N], noise1 [R,S+N]) as fp64 torch tensors, None where ops.render_draws returns None."""
    blocks = render_draws_blocks(seed, call, R, S, N, jitter, noise, importance)
    shapes = ((R, S), (R, S), (R, N), (R, S + N))
    out = []
    for i, (b, shape) in enumerate(zip(blocks, shapes)):
        if b is None:
            out.append(None)
            continue
        # whole blocks, then cut: the last normal of a ragged tail still pairs with a word of its block that no element shows
        v = (uniform_from_word if i in (0, 2) else normals_from_words)(b.reshape(-1))[:shape[0] * shape[1]]
        out.append(torch.from_numpy(v.reshape(shape)))
    return tuple(out)


def find_edge_calls(seed=1234, R=4, S=64, max_calls=1 << 21, chunk=1 << 13):
    """The search behind EDGE_CALLS: the first call numbers (N = 0: t_rand then noise0, R S / 4 blocks each) in which a word
    >= 0xFFFFFF00 lands in t_rand, a word < 0x100 lands in t_rand, and a word >= 0xFFFFFF00 lands in a normal's u0 slot (words
    0 and 2 of a noise0 block).  Returns {name: (call, flat element index, word)}."""
    q = (R * S + 3) // 4
    b = np.arange(2 * q, dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    found = {}
    for c0 in range(1, max_calls, chunk):
        calls = np.arange(c0, c0 + chunk, dtype=np.uint64)
        ctr = np.stack(np.broadcast_arrays(b[None, :] & _LO, b[None, :] >> _S32, calls[:, None] & _LO, calls[:, None] >> _S32), -1)
        w = philox4x32_10(ctr, key)                          # [chunk, 2q, 4]
        t = w[:, :q].reshape(chunk, -1)[:, :R * S]
        u0 = w[:, q:, 0::2].reshape(chunk, -1)
        for name, hit in (("t_rand_high", t >= 0xFFFFFF00), ("t_rand_low", t < 0x100), ("normal_u0_high", u0 >= 0xFFFFFF00)):
            if name not in found and hit.any():
                i, j = np.argwhere(hit)[0]
                found[name] = (int(calls[i]), int(j), int((t if name.startswith("t_") else u0)[i, j]))
        if len(found) == 3:
            break
    return found


# seed 1234, R = 4, S = 64, N = 0 (find_edge_calls(); tests/test_render_tail_port.py re-derives the words from these numbers)
EDGE_SEED, EDGE_R, EDGE_S = 1234, 4, 64
EDGE_CALLS = {"t_rand_high": 222253, "t_rand_low": 156681, "normal_u0_high": 353979}


# ------------------------------------------------------------------------------------------ compositing backward
def _opt(ups, key, shape, absolute):
    t = ups.get(key)
    if t is None:
        return torch.zeros(shape, dtype=torch.float64)
    t = t.double().reshape(shape)
    return t.abs() if absolute else t


def composite_backward_closed(raw, z, d, noise, std, white, ups, absolute=False):
    """d loss / d raw [R,S,C] in fp64 from the closed form in the comment above composite_backward_kernel:
        gw_j      = g_weights_j + g_rgb . sigmoid(c_j) + g_sem . s_j + G_depth z_j + G_acc
        dL/da_i   = gw_i T_i - (1 / t_i) sum_{j>i} gw_j w_j        (w_j = a_j T_j, T_j = prod_{i<j} t_i, t_i = 1 - a_i + 1e-10)
        g_sigma_i = dL/da_i dist_i exp(-relu(sigma_i) dist_i) [sigma_i > 0]
        g_c_i     = g_rgb w_i sig (1 - sig),   g_s_i = g_sem w_i
    G_depth / G_acc collect the per-ray terms: rays with acc <= 1e-10 take no gradient through depth or disp (depth is replaced
    by 1e10 there), disp = 1 / q with q = depth / acc gives gq = -g_disp / q^2, G_depth += gq / acc, G_acc -= gq depth / acc^2 where
    q > 1e-10, and a white background adds 1 - acc to rgb and semantics.  `ups` maps rgb / semantics / depth / acc / disp / weights
    to upstream gradients (missing or None = zero); sigma = raw[..., 3] + noise * std.
    absolute=True: every product that is summed is replaced by its absolute value (the minus of dL/da and of the white
    background become a plus) -- the term magnitude mag[R,S,C] that a rounding error of the fp32 evaluation scales with."""
    raw, z, d = raw.double(), z.double(), d.double()
    R, S, C = raw.shape
    A = torch.abs if absolute else (lambda t: t)
    sgn = 1.0 if absolute else -1.0
    norm = torch.sqrt((d * d).sum(-1, keepdim=True))
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 1e10, dtype=torch.float64)], -1) * norm
    sigma = raw[..., 3] + (noise.double() * float(std) if noise is not None else 0.0)
    e = torch.exp(-torch.relu(sigma) * dist)
    a = 1.0 - e
    t = 1.0 - a + 1e-10
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=torch.float64), t], -1), -1)[:, :-1]
    w = a * T
    sig, sem = torch.sigmoid(raw[..., :3]), raw[..., 4:]
    acc, dep = w.sum(-1), (w * z).sum(-1)
    empty = acc <= 1e-10

    g_rgb, g_sem = _opt(ups, "rgb", (R, 3), absolute), _opt(ups, "semantics", (R, C - 4), absolute)
    g_w = _opt(ups, "weights", (R, S), absolute)
    G_acc = _opt(ups, "acc", (R,), absolute)
    G_dep = torch.where(empty, torch.zeros(R, dtype=torch.float64), _opt(ups, "depth", (R,), absolute))
    acc_s = torch.where(empty, torch.ones_like(acc), acc)
    q = dep / acc_s
    through_disp = ~empty & (q > 1e-10)
    gq = torch.where(through_disp, -_opt(ups, "disp", (R,), False) / torch.where(through_disp, q * q, torch.ones_like(q)), torch.zeros_like(q))
    G_dep = G_dep + A(gq / acc_s)
    G_acc = G_acc + A(-gq * dep / (acc_s * acc_s))
    if white:
        G_acc = G_acc + sgn * (g_rgb.sum(-1) + g_sem.sum(-1))
    gw = g_w + (g_rgb[:, None, :] * sig).sum(-1) + (g_sem[:, None, :] * A(sem)).sum(-1) + G_dep[:, None] * A(z) + G_acc[:, None]
    gww = gw * w
    suffix = torch.cat([torch.flip(torch.cumsum(torch.flip(gww[:, 1:], [-1]), -1), [-1]), torch.zeros(R, 1, dtype=torch.float64)], -1)
    dLda = gw * T + sgn * suffix / t
    g_sigma = dLda * dist * e * (sigma > 0).double()
    g_c = g_rgb[:, None, :] * w[..., None] * (sig * (1.0 - sig))
    g_s = g_sem[:, None, :] * w[..., None]
    return torch.cat([g_c, g_sigma[..., None], g_s], -1)


def group_scale(mag):
    """M [R,S,C]: per ray and column group (colour 0..2, sigma 3, semantics 4..) the maximum of mag over the ray's samples and the
    group's columns, broadcast back to every element."""
    out = torch.empty_like(mag)
    for lo, hi in ((0, 3), (3, 4), (4, mag.shape[-1])):
        if hi > lo:
            out[..., lo:hi] = mag[..., lo:hi].amax(dim=(1, 2), keepdim=True)
    return out


UPSTREAMS = ("rgb", "semantics", "depth", "acc", "disp", "weights")
COMPOSITE_S = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300, 512)   # both edges of IPL = 1, 2, 3, 4, 8
COMPOSITE_C = (4, 5, 6, 7, 9, 12)                                          # NS = 2: 4, 5, 6;  NS = 8: 7, 9, 12
COMPOSITE_R = 37
# (S, C, regime) -> seed increment where the default seed draws a ray that is ill-conditioned in fp32 itself: its first sample with
# sigma > 0 is almost opaque, so every sigma gradient of the ray hangs on t = 1 - alpha ~ 1e-7, which fp32 holds to a per cent (the
# reference's own fp32 autograd is 1e4..2e5 units off there); and three 512-sample cases above 200 units (see the CPU test)
SEED_MOVES = {(63, 6, "dense"): 1, (63, 7, "dense"): 1, (64, 4, "dense"): 2, (512, 4, "thin"): 3, (512, 6, "thin"): 4,
              (512, 7, "thin"): 1, (512, 12, "dense"): 1}
REF_WORST = 188.31         # worst error of the reference's fp32 autograd over the case list, in units of 2^-24 M (the CPU test measures it)
COMPOSITE_K = 4 * REF_WORST


def composite_configs(S):
    """The 12 (C, regime, white, noisy) configurations run at S samples: every C in both sigma regimes; background and noise
    rotate so that each S sees every (white, noisy) pair three times and each (C, regime) sees all four over the S list."""
    i0 = COMPOSITE_S.index(S)
    out = []
    for i, (C, regime) in enumerate((C, regime) for C in COMPOSITE_C for regime in ("dense", "thin")):
        k = (i + i0) & 3
        out.append((C, regime, bool(k & 1), bool(k & 2)))
    return out


def composite_case(S, C, regime, white, noisy):
    """fp32 inputs of one configuration: dict(raw, z, d, noise, std, white, ups).  `dense` is the sigma of
    test_composite_backward_vs_autograd (3 N(0,1) + 0.5: nearly every ray opaque); `thin` is N(0,1) 12/S + 4/S with every second ray
    ending on sigma = -0.5, so acc stays well inside (0, 1) and g_acc matters.  Ray 0 is empty and ray 1 has an opaque sample.
    The depths span 13 S/64 below 64 samples (the existing test's 13 from there on): at S = 2 a 13-long interval times sigma ~ 10
    puts exp(-sigma dist) below the smallest fp32 number, where a bound in units of the ray's own magnitude means nothing."""
    R = COMPOSITE_R
    g = torch.Generator().manual_seed(100000 * (regime == "thin") + S * 100 + C + 1000003 * SEED_MOVES.get((S, C, regime), 0))
    raw = torch.randn(R, S, C, generator=g)
    if regime == "dense":
        raw[..., 3] = raw[..., 3] * 3 + 0.5
    else:
        raw[..., 3] = raw[..., 3] * (12.0 / S) + 4.0 / S
        raw[2::2, -1, 3] = -0.5
    raw[0, :, 3] = -1.0                      # empty ray: acc = 0, depth -> 1e10 (no gradient through depth / disp)
    raw[1, min(3, S - 1), 3] = 80.0          # opaque sample
    z = torch.sort(1.2 + 13 * min(1.0, S / 64) * torch.rand(R, S, generator=g), -1)[0]
    d = torch.randn(R, 3, generator=g)
    noise = std = None
    if noisy:
        noise = torch.randn(R, S, generator=g) * (1.0 if regime == "dense" else 8.0 / S)
        std = 0.75
    ups = dict(rgb=torch.randn(R, 3, generator=g), depth=torch.randn(R, 1, generator=g), acc=torch.randn(R, 1, generator=g),
               disp=torch.randn(R, 1, generator=g) * 0.1, weights=torch.randn(R, S, generator=g))
    if C > 4:
        ups["semantics"] = torch.randn(R, C - 4, generator=g)
    ups["disp"][0] = 0.0                     # the reference's autograd gives NaN for an empty ray with g_disp != 0
    return dict(raw=raw, z=z, d=d, noise=noise, std=std or 0.0, white=white, ups=ups)


def upstream_sets(ups):
    """All upstream gradients together, then each one alone (the others None)."""
    return [("all", dict(ups))] + [(k, {k: ups[k]}) for k in UPSTREAMS if k in ups]


# ------------------------------------------------------------------------------------------ ray-gradient reduce
def ray_grad_reduce_closed(g_pts, g_dirs, z, d, raw, g_raw, noise, std):
    """(g_o, g_d, Y_o, Y_d), each [R,3] fp64: the closed form in the comment above ray_grad_reduce_kernel,
        g_o = sum_s g_pts,   g_d = sum_s z_s g_pts + (g_v - v (v . g_v)) / |d| + g_n v,    v = d / |d|,
        g_v = sum_s g_dirs,  g_n = sum_s g_raw3_s relu(raw3_s + noise_s std) / |d|,
    and the magnitudes of what they sum,
        Y_o_c = sum_s |g_pts_c|
        Y_d_c = sum_s |g_pts_c| |z| + (sum_s |g_dirs_c| + |v_c| sum_k |v_k| sum_s |g_dirs_k|) / |d|
                + |v_c| / |d| sum_s |g_raw3| (|raw3| + |noise| std)."""
    g_pts, z, d, raw, g_raw = (t.double() for t in (g_pts, z, d, raw, g_raw))
    R, S = z.shape
    g_pts = g_pts.reshape(R, S, 3)
    g_dirs = torch.zeros_like(g_pts) if g_dirs is None else g_dirs.double().reshape(R, S, 3)
    nz = torch.zeros(R, S, dtype=torch.float64) if noise is None else noise.double() * float(std)
    n = torch.sqrt((d * d).sum(-1, keepdim=True))
    v = d / n
    g_v = g_dirs.sum(1)
    g_n = (g_raw[..., 3] * torch.relu(raw[..., 3] + nz)).sum(-1, keepdim=True) / n
    g_o = g_pts.sum(1)
    g_d = (g_pts * z[..., None]).sum(1) + (g_v - v * (v * g_v).sum(-1, keepdim=True)) / n + g_n * v
    a_v = g_dirs.abs().sum(1)
    Y_o = g_pts.abs().sum(1)
    Y_d = ((g_pts.abs() * z.abs()[..., None]).sum(1) + (a_v + v.abs() * (v.abs() * a_v).sum(-1, keepdim=True)) / n
           + v.abs() / n * (g_raw[..., 3].abs() * (raw[..., 3].abs() + nz.abs())).sum(-1, keepdim=True))
    return g_o, g_d, Y_o, Y_d


RAYGRAD_R, RAYGRAD_S, RAYGRAD_C, RAYGRAD_SCALE = (1, 7, 37), (1, 50, 63, 64, 65, 192, 300), (4, 6, 12), (0.01, 1.0, 30.0)


def raygrad_case(R, S, C, scale, seed):
    """fp32 inputs of one ray_grad_reduce case: dict(g_pts, g_dirs, z, d, raw, g_raw, noise); every third row has sigma <= 0
    throughout, noise or not."""
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(1.2 + 13 * torch.rand(R, S, generator=g), -1)[0]
    d = torch.randn(R, 3, generator=g) * scale
    raw = torch.randn(R, S, C, generator=g)
    noise = torch.randn(R, S, generator=g)
    raw[::3, :, 3] = -8.0 - raw[::3, :, 3].abs()
    noise[::3] = noise[::3].clamp(-4.0, 4.0)
    return dict(g_pts=torch.randn(R * S, 3, generator=g) * 512.0, g_dirs=torch.randn(R * S, 3, generator=g), z=z, d=d, raw=raw,
                g_raw=torch.randn(R, S, C, generator=g), noise=noise)
