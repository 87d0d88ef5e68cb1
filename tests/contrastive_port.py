"""TEST INFRASTRUCTURE -- plain CPU references for csrc/contrastive.hip (numpy / torch, no GPU):

* ``sim_emulated``    <- the arithmetic the comments in contrastive_kernel / similarity_negatives_kernel state: norms from an fp64 sum
                        rounded once and clamped at 1e-8, both vectors normalised FIRST, every quotient and product rounded to fp32, the
                        sum of the products in fp64, rounded once.  Only the order of the fp64 additions is free.
* ``sim_fp64``        <- the same cosine matrix with nothing rounded.
* ``closed_form``     <- fp64 loss = -log(mx / (mx + mn)) and d loss / d e for GIVEN picks, from d sim_ij / d e_i = (e^_j - sim_ij e^_i) / n_i.
* ``first_extremes``  <- first-occurrence arg-max / arg-min over the off-diagonal entries in row-major order (sim[~eye] then
                        torch.argmax / argmin, utils/image.py:205-208): a NaN wins, and the first one at that.
* ``cases``           <- the seeded inputs of tests/test_gpu_contrastive_edges.py, drawn as tests/golden/make_goldens_contrastive.py draws.

tests/test_contrastive_port.py validates all of it on the CPU (fp64 autograd of oracle/losses_port.nerf_contrastive); the GPU tests
hold the kernels to it.
"""
import numpy as np
import torch

U24 = 2.0 ** -24          # one unit of the bounds: half an fp32 ulp of 1
SIM_BOUND = 4 * U24       # |fp32-arithmetic cosine - exact cosine|: three roundings per product of normalised vectors (the two
#                           quotients, the product; Cauchy-Schwarz keeps sum |e^_ik e^_jk| <= 1) plus the final rounding of the sum
EPS = 1e-8                # F.cosine_similarity's eps
GAP = 1e-4                # the extremes of every case are this far from the next distinct value

# (B, D, common, seed): B at 2 / 3 / 4 (one shared entry / a shared row / four rows), across the 4-wave stride, at the limit 120;
# D ragged against the 64-lane stride (63 / 65 / 257), past one 256-thread pass of the gradient loop (257 / 384 / 1000), tiny (5 / 7)
CASES = [(2, 384, 3.0, 1), (3, 384, 3.0, 1), (4, 7, 2.0, 5), (16, 63, 2.0, 1), (33, 64, 2.0, 1), (65, 65, 2.0, 1), (100, 257, 3.0, 1),
         (120, 384, 3.0, 1), (120, 1000, 3.0, 2), (120, 5, 2.0, 1)]
# seeds: 1, except (120, 1000), whose max gap at seed 1 is 9.6e-6, and (4, 7), where 5 is the first seed at which the two pairs are
# disjoint (four rows carry gradient; at seeds 1-4 they share a token, which B = 3 covers)


def case_id(case):
    return "B%d_D%d" % case[:2]


def draw(B, D, common, seed):
    """randn(B, D) + common * randn(1, D): class tokens of crops of one scene share a component (similarities positive and close)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=g) + common * torch.randn(1, D, generator=g)


def cases():
    return [(c, draw(*c)) for c in CASES]


def _np32(e):
    return np.ascontiguousarray(e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else e, dtype=np.float32)


def sim_fp64(e):
    e = np.asarray(e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else e, dtype=np.float64)
    n = np.maximum(np.sqrt((e * e).sum(-1)), EPS)
    h = e / n[:, None]
    s = np.triu(h @ h.T)
    return s + np.triu(s, 1).T                                      # symmetric bit for bit, whatever the BLAS does


def sim_emulated(e):
    """[B,B] float32, the kernels' arithmetic (see the module docstring)."""
    e = _np32(e)
    B = e.shape[0]
    e64 = e.astype(np.float64)
    n = np.maximum(np.sqrt((e64 * e64).sum(-1)).astype(np.float32), np.float32(EPS))
    h = e / n[:, None]                                              # fp32 quotients
    assert h.dtype == np.float32
    out = np.empty((B, B), dtype=np.float32)
    for i in range(B):
        prod = h[i][None, :] * h                                    # fp32 products
        assert prod.dtype == np.float32
        out[i] = prod.astype(np.float64).sum(-1).astype(np.float32)
    return out


def sim_fp32_lanes(e):
    """What the kernels would return if each of the 64 lanes accumulated its share of a pair sum (k = lane, lane + 64, ...) in fp32
    and only the lanes were added in fp64 -- the arithmetic the kernels must NOT have.  tests/test_contrastive_port.py uses it to
    show that the inputs of stress_cases() tell the two apart."""
    e = _np32(e)
    B, D = e.shape
    e64 = e.astype(np.float64)
    n = np.maximum(np.sqrt((e64 * e64).sum(-1)).astype(np.float32), np.float32(EPS))
    h = e / n[:, None]
    out = np.empty((B, B), dtype=np.float32)
    for i in range(B):
        prod = h[i][None, :] * h
        lanes = np.zeros((B, 64), dtype=np.float32)
        for k0 in range(0, D, 64):
            blk = prod[:, k0:k0 + 64]
            lanes[:, :blk.shape[1]] = lanes[:, :blk.shape[1]] + blk
        out[i] = lanes.astype(np.float64).sum(-1).astype(np.float32)
    return out


def loss_from_matrix(sim, picks):
    """The tail of contrastive_kernel on a given fp32 matrix: sum and quotient in fp32, the logarithm in fp64, rounded once."""
    mx, mn = sim[picks[0], picks[1]], sim[picks[2], picks[3]]
    with np.errstate(all="ignore"):
        q = np.float32(mx / np.float32(mx + mn))
        return np.float32(-np.log(np.float64(q)))


def ulps(a, b):
    """Distance in fp32 units in the last place, elementwise (finite values, either sign)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def stress_cases():
    """Two inputs at D = 1000 on which the PRECISION of the pair sums shows in the outputs.  Coordinates 0 and 960 are the first and
    the last element of lane 0's share; they carry most of each token's norm, so lane 0 holds a partial sum of ~0.3 - 0.8 while the
    fourteen small products between them are added.
    * "cancel": 8 uncorrelated tokens with e[:, 0] = 40 and e[:, 960] = +-40 alternating.  For tokens of opposite sign the two big
      products cancel and the cosine is ~0.01: rounding the small products at the partial sum's ulp is tens to hundreds of ulps there.
    * "near_zero_sum": 4 tokens whose (e_0, e_960) = 60 (cos t, sin t) with t = 0, 0.1, pi + 0.35, 1.5: max = cos(0.1) a and
      min = -cos(0.25) a leave max + min ~ 0.02, so an error of 1e-7 in either is 5e-6 in the loss (ulp 2.4e-7)."""
    g = torch.Generator().manual_seed(2)
    a = torch.randn(8, 1000, generator=g)
    a[:, 0] = 40.0
    a[:, 960] = 40.0 * torch.tensor([1.0, -1.0] * 4)
    g = torch.Generator().manual_seed(4)
    b = torch.randn(4, 1000, generator=g)
    t = torch.tensor([0.0, 0.1, np.pi + 0.35, 1.5], dtype=torch.float64)
    b[:, 0] = (60.0 * torch.cos(t)).float()
    b[:, 960] = (60.0 * torch.sin(t)).float()
    return [("cancel", a), ("near_zero_sum", b)]


def first_extremes(sim):
    """(i_max, j_max, i_min, j_min) of a [B,B] matrix, B >= 2."""
    sim = np.asarray(sim.detach().cpu().numpy() if isinstance(sim, torch.Tensor) else sim)
    B = sim.shape[0]
    flat = np.flatnonzero(~np.eye(B, dtype=bool).reshape(-1))       # row-major, diagonal skipped
    v = sim.reshape(-1)[flat]
    nan = np.flatnonzero(np.isnan(v))
    if nan.size:
        k_max = k_min = int(nan[0])
    else:
        k_max, k_min = int(np.argmax(v)), int(np.argmin(v))         # first occurrence
    a, b = int(flat[k_max]), int(flat[k_min])
    return a // B, a % B, b // B, b % B


def closed_form(e64, i_max, j_max, i_min, j_min):
    """(loss, grad [B,D], mx, mn) in fp64 for the given picks."""
    e = np.asarray(e64.detach().cpu().numpy() if isinstance(e64, torch.Tensor) else e64, dtype=np.float64)
    n = np.maximum(np.sqrt((e * e).sum(-1)), EPS)
    h = e / n[:, None]
    mx, mn = float(h[i_max] @ h[j_max]), float(h[i_min] @ h[j_min])
    loss = -np.log(mx / (mx + mn))
    grad = np.zeros_like(e)
    # d loss / d mx = -(1/mx - 1/(mx+mn)), d loss / d mn = 1/(mx+mn)
    for (i, j, s, c) in ((i_max, j_max, mx, -(1.0 / mx - 1.0 / (mx + mn))), (i_min, j_min, mn, 1.0 / (mx + mn))):
        grad[i] += c * (h[j] - s * h[i]) / n[i]
        grad[j] += c * (h[i] - s * h[j]) / n[j]
    return float(loss), grad, mx, mn


def loss_bound(mx, mn, loss):
    """|kernel loss - closed_form loss| for equal picks: mx and mn each off by at most SIM_BOUND, propagated through
    d loss / d mx and d loss / d mn, plus the fp32 roundings of the sum, the quotient, the logarithm and the result."""
    return (abs(1.0 / mx - 1.0 / (mx + mn)) + 1.0 / (mx + mn)) * SIM_BOUND + 2.0 ** -22 * abs(loss)


def offdiag_gaps(sim64):
    """(gap below the maximum, gap above the minimum, max + min) over the distinct off-diagonal values of a symmetric matrix
    (the mirror entry (j, i) of (i, j) is the same value, not a competitor)."""
    B = sim64.shape[0]
    v = np.unique(sim64[np.triu_indices(B, 1)])
    if v.size == 1:
        return np.inf, np.inf, float(2 * v[0])
    return float(v[-1] - v[-2]), float(v[1] - v[0]), float(v[-1] + v[0])


def port_loss_and_grad(e, dtype):
    """oracle/losses_port.nerf_contrastive and its autograd in `dtype` -> (loss, grad) as fp64 numpy."""
    from oracle import losses_port as lp
    a = e.detach().cpu().to(dtype).clone().requires_grad_(True)
    loss = lp.nerf_contrastive(a)
    loss.backward()
    return float(loss.detach().double()), a.grad.double().numpy()
