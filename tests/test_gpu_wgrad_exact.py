"""The weight-gradient reductions (csrc/wgrad.hip, the semantic head's in csrc/backward.hip and csrc/sem_wgrad16.hip) and the ReLU mask,
every dispatch, against fp64 -- with ZERO tolerance.

The kernels are fed small integers (fp32 G, fp32 / fp16 X): every product is an integer, every partial sum stays below 2^24 and is
therefore exact in fp32 under ANY summation order, the split-fp16 operands have lo = 0 and the fp64 combine of the partials is exact.
So dW must equal G.double().T @ X.double() and db must equal G.double().sum(0) bit for bit: one point dropped or counted twice in a
ragged tail, one k-subset's partial missing, one misplaced accumulator element changes an integer.  Each case asserts the < 2^24
condition (on |G|^T |X|) before it compares.  A planner in plain Python mirrors the host arithmetic and the kernels' range split; a
CPU test holds the point counts used here to the branches they have to reach.  One test with real data (rows and columns decades
apart) holds every ELEMENT to the worst-case bound of fp32 accumulation, the only tolerances in this file.

(The GPU tests carry the `gpu` mark one by one, not through a module-wide pytestmark: the planner's coverage test has to run on a
machine without a GPU.)
"""
import ctypes as C
import functools

import pytest
import torch

import nerf_sos_amd  # noqa: F401
from nerf_sos_amd import _lib, ops

gpu = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (32, 64, 128, 256)
EXACT = float(2 ** 24)          # integers below this are exact in fp32


# ---- planners: the host arithmetic of wgrad_entry / wgrad_x3_entry and the kernels' range split, in plain Python -----------------
# Constants of csrc/wgrad.hip:
#   kWgradMaxBlocks = 256;  MT = M / 32, RW = min(MT, 4) row groups, KW = 4 / RW interleaved point subsets, RT = MT / RW, NT = N / 32;
#   U = 4 (NSOS_WG_U) for RT * NT >= 16, 6 for RT * NT >= 8, else 8 k-steps per operand group;
#   blocks = min(256, max(1, ceil(P / (2 KW))));  chunk = ceil(P / blocks) rounded up to a multiple of 2 KW;
#   workgroup b owns points [b chunk, min(b chunk + chunk, P)); its k-subset kw the k-steps at base + j * 2 KW + {0, 1}, base = start + 2 kw.
#   wgrad_x3_kernel: 16-point steps, blocks = min(256, max(1, ceil(P / 16))), per = ceil(steps / blocks) steps per workgroup.
MAX_BLOCKS = 256


def wgrad_consts(M, N):
    MT = M // 32
    RW = min(MT, 4)
    KW = 4 // RW
    RT, NT = MT // RW, N // 32
    U = 4 if RT * NT >= 16 else (6 if RT * NT >= 8 else 8)
    return KW, U


def wgrad_plan(M, N, P):
    """What wgrad_kernel<RT, NT, XT> does with P points: the set of n_grp values over all (workgroup, k-subset) pairs, whether a
    half-valid last k-step occurs, whether a workgroup without any point occurs, the block count and the longest per-wave run of
    points (the number of terms one fp32 accumulator element sums)."""
    KW, U = wgrad_consts(M, N)
    step = 2 * KW
    units = (P + step - 1) // step
    blocks = min(MAX_BLOCKS, max(units, 1))
    chunk = (P + blocks - 1) // blocks
    chunk = (chunk + step - 1) // step * step
    n_grp, half, empty, longest = set(), False, False, 0
    for b in range(blocks):
        start = b * chunk
        end = start + chunk if start + chunk < P else P
        if end <= start:
            empty = True
        for kw in range(KW):
            base = start + 2 * kw
            n_ks = (end - base + step - 1) // step if base < end else 0
            n_full = (end - 2 - base) // step + 1 if base + 1 < end else 0
            assert n_ks - n_full in (0, 1)
            n_grp.add(n_full // U)
            half |= n_ks > n_full
            longest = max(longest, 2 * n_full + (n_ks - n_full))
    return dict(KW=KW, U=U, blocks=blocks, n_grp=n_grp, half=half, empty=empty, longest=longest)


def wgrad_x3_plan(P):
    """What wgrad_x3_kernel does with P points: per workgroup the number nf of full 16-point steps and whether the ragged step follows."""
    steps = (P + 15) // 16
    blocks = min(MAX_BLOCKS, max(steps, 1))
    per = (steps + blocks - 1) // blocks
    full_all = P // 16
    nf_set, ragged_after, empty, longest = set(), set(), False, 0
    for b in range(blocks):
        s0 = b * per
        s1 = s0 + per if s0 + per < steps else steps
        f1 = min(s1, full_all)
        ragged = s1 > f1 and s1 > s0
        nf = max(f1 - s0, 0)
        if s1 <= s0:
            empty = True
            continue
        nf_set.add(nf)
        if ragged:
            ragged_after.add(nf)
        longest = max(longest, 16 * nf + (P - 16 * f1 if ragged else 0))
    return dict(blocks=blocks, nf=nf_set, ragged_after=ragged_after, empty=empty, longest=longest)


def wgrad_points(M, N):
    """The point counts of one (M, N): T = 256 * 2 KW * U points give every wave exactly one operand group.  T + 1: one group + a
    one-step tail, fewer workgroups than launched (empty ones), a lone last point; 2 T - 1: two groups, the last wave one group and
    a half-valid step; 3 T: three groups, no tail.  Then the smallest counts and both sides of the block count reaching 256."""
    KW, U = wgrad_consts(M, N)
    s = 2 * KW
    T = MAX_BLOCKS * s * U
    return sorted({T + 1, 2 * T - 1, 3 * T, 0, 1, 2, 3, s - 1, s, s + 1, (MAX_BLOCKS - 1) * s, (MAX_BLOCKS - 1) * s + 1})


def wgrad_main_point(M, N):
    KW, U = wgrad_consts(M, N)
    return MAX_BLOCKS * 2 * KW * U + 1


# per = 2, 3, 4 steps per workgroup, the last step ragged: nf = per in all workgroups but the last, per - 1 and the ragged step there;
# 257 steps (4097, 4112): per = 2, 129 workgroups with steps, 127 without
X3_POINTS = sorted({2 * 4096 - 11, 3 * 4096 - 11, 4 * 4096 - 11, 0, 1, 15, 16, 17, 31, 32, 33, 4096, 4097, 4112})


def test_point_counts_reach_every_branch():
    """CPU: the planner says the point counts of each (M, N) reach every code path of wgrad_kernel, and X3_POINTS every one of
    wgrad_x3_kernel."""
    for M in SIZES:
        for N in SIZES:
            plans = [wgrad_plan(M, N, P) for P in wgrad_points(M, N)]
            grp = set().union(*(p["n_grp"] for p in plans))
            assert 0 in grp, (M, N)                                              # tail only
            assert any(g & 1 for g in grp), (M, N)                               # the odd last group after the pair loop
            assert any(g >= 2 and not g & 1 for g in grp), (M, N)                # the pair loop alone
            assert any(p["half"] for p in plans), (M, N)
            assert any(p["empty"] for p in plans), (M, N)
            assert any(p["blocks"] < MAX_BLOCKS for p in plans) and any(p["blocks"] == MAX_BLOCKS for p in plans), (M, N)
            assert {p["blocks"] for p in plans} >= {MAX_BLOCKS - 1, MAX_BLOCKS}, (M, N)
            # the pipelined loop's counts in one plan each, so that no branch is reached only together with another
            T1, T2, T3 = (wgrad_plan(M, N, k * (wgrad_main_point(M, N) - 1) + d) for k, d in ((1, 1), (2, -1), (3, 0)))
            assert 1 in T1["n_grp"] and T1["half"] and T1["empty"], (M, N)
            assert {1, 2} <= T2["n_grp"] and T2["half"] and not T2["empty"], (M, N)
            assert T3["n_grp"] == {3} and not T3["half"] and not T3["empty"], (M, N)
            assert max(p["longest"] for p in plans) == 3 * 2 * T3["U"]   # a wave sums at most 3 groups of U k-steps of 2 points
    assert max(max(wgrad_points(M, N)) for M in SIZES for N in SIZES) <= PMAX
    plans = {P: wgrad_x3_plan(P) for P in X3_POINTS}
    nf = set().union(*(p["nf"] for p in plans.values()))
    assert {0, 1, 2, 3, 4} <= nf
    after = set().union(*(p["ragged_after"] for p in plans.values()))
    assert 0 in after and any(a & 1 for a in after) and any(a >= 2 and not a & 1 for a in after)
    assert any(p["empty"] for p in plans.values())
    assert plans[0]["nf"] == set() and plans[0]["empty"]                   # P = 0: one workgroup, no step
    assert plans[4097]["ragged_after"] == {0} and plans[4097]["empty"] and plans[4112]["empty"]
    assert plans[3 * 4096 - 11]["ragged_after"] == {2} and plans[4 * 4096 - 11]["ragged_after"] == {3}
    assert max(X3_POINTS) <= PMAX


# ---- shared integer data and its fp64 results ---------------------------------------------------------------------------
PMAX = 3 * MAX_BLOCKS * 8 * 8        # the largest point count above: 3 T for KW = 4, U = 8
SENT = -12345.0                      # pre-fill of everything a call must not write


def _ints_host():
    """G in -3..3, X in 0..7 (ReLU-like), about half of each zero: |dW| <= 3 * 7 * PMAX = 1.0e6 < 2^24."""
    g = torch.Generator().manual_seed(20240)
    Gi = torch.randint(-3, 4, (PMAX, 256), generator=g) * (torch.rand(PMAX, 256, generator=g) < 0.5)
    Xi = torch.randint(0, 8, (PMAX, 256), generator=g) * (torch.rand(PMAX, 256, generator=g) < 0.5)
    return Gi.float(), Xi.float()


@functools.lru_cache(maxsize=None)
def _ints():
    """The integers on the device.  Made once, never written."""
    return tuple(t.to(DEV) for t in _ints_host())


@functools.lru_cache(maxsize=None)
def _want(P):
    """fp64 results over the first P points for the full 256 x 256 block (every (M, N) case is its leading sub-block):
    (dW, db, |G|^T |X|, sum |G|)."""
    Gi, Xi = _ints()
    Gd, Xd = Gi[:P].double(), Xi[:P].double()
    return Gd.T @ Xd, Gd.sum(0), Gd.abs().T @ Xd.abs(), Gd.abs().sum(0)


def _operands(M, N, xdtype, P):
    """G [P, M] and X [P, N] as column slices at odd offsets of taller, wider buffers that hold NaN everywhere else."""
    Gi, Xi = _ints()
    Gw = torch.full((P + 3, 300), float("nan"), device=DEV)
    Xw = torch.full((P + 3, N + 10), float("nan"), device=DEV, dtype=xdtype)
    Gw[:P, 7:7 + M] = Gi[:P, :M]
    Xw[:P, 3:3 + N] = Xi[:P, :N].to(xdtype)
    return Gw[:P, 7:7 + M], Xw[:P, 3:3 + N]


def _outputs(M, N):
    Ww = torch.full((M + 2, N + 11), SENT, device=DEV)
    bw = torch.full((M + 16,), SENT, device=DEV)
    return Ww, bw, Ww[1:1 + M, 5:5 + N], bw[8:8 + M]


def _untouched(Ww, bw, M, N, bias=True):
    Wc, bc = Ww.clone(), bw.clone()
    Wc[1:1 + M, 5:5 + N] = SENT
    if bias:
        bc[8:8 + M] = SENT
    return bool((Wc == SENT).all()) and bool((bc == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_exact(M, N, xdtype, P, split, with_none):
    wW, wb, A, Ab = _want(P)
    assert float(A[:M, :N].max()) < EXACT and float(Ab[:M].max()) < EXACT, "the inputs do not keep the partial sums exact"
    wantW, wantb = wW[:M, :N].float(), wb[:M].float()
    G, X = _operands(M, N, xdtype, P)
    Ww, bw, dW, db = _outputs(M, N)
    ops.wgrad(G, X, dW, db, split_fp16=split)
    assert torch.equal(dW, wantW), f"dW: {int((dW != wantW).sum())} elements differ from fp64"
    assert torch.equal(db, wantb), f"db: {int((db != wantb).sum())} elements differ from fp64"
    assert _untouched(Ww, bw, M, N), "wrote outside dW / db"
    Ww2, bw2, dW2, db2 = _outputs(M, N)
    ops.wgrad(G, X, dW2, db2, split_fp16=split)
    assert torch.equal(_bits(dW), _bits(dW2)) and torch.equal(_bits(db), _bits(db2)), "not deterministic"
    if P == 0:
        assert not dW.any() and not db.any()
    if with_none:
        Ww3, bw3, dW3, _ = _outputs(M, N)
        ops.wgrad(G, X, dW3, None, split_fp16=split)
        assert torch.equal(dW3, wantW) and _untouched(Ww3, bw3, M, N, bias=False) and bool((bw3 == SENT).all())
    return dW, db


_DT = {"f32": torch.float32, "f16": torch.float16}
CASES = [(M, N, x, P) for M in SIZES for N in SIZES for x in _DT for P in wgrad_points(M, N)]


@gpu
@pytest.mark.parametrize("M,N,xdtype,P", CASES)
def test_wgrad_exact_integers(M, N, xdtype, P):
    """nsos_wgrad / nsos_wgrad_xh, all 16 instantiations per X type: bit-equal to fp64 at every block count and tail length;
    NaN around the operands, sentinels around the outputs; one point count per shape also without a bias."""
    _check_exact(M, N, _DT[xdtype], P, False, with_none=P == wgrad_main_point(M, N))


@gpu
@pytest.mark.parametrize("P", X3_POINTS)
@pytest.mark.parametrize("xdtype", list(_DT))
def test_wgrad_x3_exact_integers(xdtype, P):
    """nsos_wgrad_x3 / nsos_wgrad_x3_xh: integers have no lo part, so the three-MFMA product is exact as well -- bit-equal to
    fp64 and to the exact kernel."""
    dW, db = _check_exact(256, 256, _DT[xdtype], P, True, with_none=P == 3 * 4096 - 11)
    eW, eb = _check_exact(256, 256, _DT[xdtype], P, False, with_none=False)
    assert torch.equal(_bits(dW), _bits(eW)) and torch.equal(_bits(db), _bits(eb))


@gpu
def test_wgrad_batch_exact_integers():
    """nsos_wgrad_batch: a 224-wide gradient block as 128 + 64 + 32 rows over input segments of 256 + 64 columns, inside wider
    buffers; the bias comes with the first segment's items only.  Exact over the whole flat buffer, NaN wherever no item writes."""
    P = 3001
    Gi, Xi = _ints()
    gc0, xc0, ldg, ldx, ldw = 5, 3, 224 + 13, 320 + 7, 320 + 4
    Gt = torch.full((P + 2, ldg), float("nan"), device=DEV)
    Xt = torch.full((P + 2, ldx), float("nan"), device=DEV)
    Gt[:P, gc0:gc0 + 224] = Gi[:P, :224]
    Xt[:P, xc0:xc0 + 256] = Xi[:P]
    Xt[:P, xc0 + 256:xc0 + 320] = Xi[PMAX - P:, :64]          # (the 64 extra input columns: other rows of the same integers)
    w0 = 10
    b0 = w0 + 224 * ldw + 6
    total = b0 + 224 + 9
    items = []
    for row, m in ((0, 128), (128, 64), (192, 32)):
        for xc, n in ((0, 256), (256, 64)):
            items.append((w0 + row * ldw + xc, b0 + row if xc == 0 else -1, gc0 + row, xc0 + xc, m, n, ldw))
    arr = (_lib.WgradItem * len(items))()
    for i, (w, b, gc, xc, m, n, ld) in enumerate(items):
        arr[i].w_off, arr[i].b_off, arr[i].g_col, arr[i].x_col, arr[i].M, arr[i].N, arr[i].ldw = w, b, gc, xc, m, n, ld
    flat = torch.full((total,), float("nan"), device=DEV)
    ops.wgrad_batch(arr, len(items), Gt[:P], Xt[:P], flat)
    Gd, Xd = Gt[:P, gc0:gc0 + 224].double(), Xt[:P, xc0:xc0 + 320].double()
    assert float((Gd.abs().T @ Xd.abs()).max()) < EXACT and float(Gd.abs().sum(0).max()) < EXACT
    want = torch.full((total,), float("nan"), device=DEV)
    want[w0:w0 + 224 * ldw].view(224, ldw)[:, :320] = (Gd.T @ Xd).float()
    want[b0:b0 + 224] = Gd.sum(0).float()
    assert torch.equal(torch.isnan(flat), torch.isnan(want)), "the batch wrote other elements than its items name"
    keep = ~torch.isnan(want)
    assert int(keep.sum()) == 224 * 320 + 224
    assert torch.equal(flat[keep], want[keep])
    again = torch.full((total,), float("nan"), device=DEV)
    ops.wgrad_batch(arr, len(items), Gt[:P], Xt[:P], again)
    assert torch.equal(_bits(flat), _bits(again))


@gpu
@pytest.mark.parametrize("n_pts,n_cols", [(37, 20), (1001, 36), (0, 20)])
def test_relu_mask_bitwise(n_pts, n_cols):
    """nsos_relu_mask on column slices: h with both zeros, subnormals, infinities and NaN; g random BITS (NaN payloads included):
    g's bits survive where h > 0, +0.0 elsewhere; nothing outside the slice moves."""
    assert (n_pts * n_cols // 4) % 256 != 0 or n_pts == 0
    gen = torch.Generator().manual_seed(7 + n_pts)
    rows, ldg, ldh = n_pts + 2, n_cols + 12, n_cols + 8
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1.1e-38, -1.1e-38, float("inf"), -float("inf"), float("nan"), -float("nan"),
                            1.0, -1.0, 3.5e38, -2.5e-7])
    hw = special[torch.randint(0, len(special), (rows, ldh), generator=gen)]
    plain = torch.randn(rows, ldh, generator=gen)
    hw = torch.where(torch.rand(rows, ldh, generator=gen) < 0.3, plain, hw)
    gw_bits = torch.randint(-2 ** 31, 2 ** 31, (rows, ldg), generator=gen, dtype=torch.int64).to(torch.int32)
    gw_bits[0, :4] = torch.tensor([0x7FC00001, -1, 0x7F800001, -0x7FFFFFFF - 1], dtype=torch.int64).to(torch.int32)   # NaNs, -0.0
    want = gw_bits.clone()
    sl = (slice(0, n_pts), slice(4, 4 + n_cols))
    want[sl] = torch.where(hw[:n_pts, 8:8 + n_cols] > 0, gw_bits[sl], torch.zeros((), dtype=torch.int32))
    gw = gw_bits.to(DEV).view(torch.float32)
    hd = hw.to(DEV)
    assert torch.equal(hd.view(torch.int32).cpu(), hw.view(torch.int32)), "the copy to the device changed h's bits"
    ret = ops.relu_mask_(gw[:n_pts, 4:4 + n_cols], hd[:n_pts, 8:8 + n_cols])
    assert ret.data_ptr() == gw[:n_pts, 4:4 + n_cols].data_ptr()
    got = gw.view(torch.int32).cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} words differ"
    assert torch.equal(hd.view(torch.int32).cpu(), hw.view(torch.int32)), "h was written"
    if n_pts:
        m = hw[:n_pts, 8:8 + n_cols] > 0
        assert bool(m.any()) and bool((~m).any())


# ---- the semantic head's fused reductions ---------------------------------------------------------------------------------
SEM_VARIANTS = ("exact", "split_f32", "split_f16", "split_bf16", "split_f16_tiled")


def _sem_host(R, S):
    """Integer-valued inputs of nsos_sem_head_wgrad[_x3] and the fp64 results of its formulas (models/renderer.py:64-66,
    models/nerf_mlp.py:61,80).  g_logits and g_hid are multiples of 1/4, and the split kernels multiply g_hid by the power of two
    that brings max|g_semantics| * max(|w2[0]| + |w2[1]|) = 3 * 4 to 2^8, i.e. by 16."""
    g = torch.Generator().manual_seed(R * 1000 + S)
    P = R * S
    weights = torch.tensor([0.0, 0.25, 0.5, 1.0, 2.0])[torch.randint(0, 5, (R, S), generator=g)]
    weights = weights * (torch.rand(R, S, generator=g) < 0.7)
    g_sem = torch.randint(-3, 4, (R, 2), generator=g).float()
    g_sem[0, 0] = 3.0
    w2 = torch.randint(-2, 3, (2, 128), generator=g).float()
    w2[:, 0] = 2.0
    hid = (torch.randint(1, 6, (P, 128), generator=g) * (torch.rand(P, 128, generator=g) < 0.3)).float()
    sem_in = (torch.randint(-3, 4, (P, 320), generator=g) * (torch.rand(P, 320, generator=g) < 0.4)).float()
    sem_in[:, 319] = 1.0
    gl = (weights.reshape(P, 1) * g_sem.repeat_interleave(S, 0)).double()
    gh = (gl @ w2.double()) * (hid > 0)
    want = (gh.T @ sem_in.double(), gl.T @ hid.double(), gl.sum(0))
    mags = (gh.abs().T @ sem_in.double().abs(), gl.abs().T @ hid.double(), gl.abs().sum(0))
    return (weights, g_sem, w2, hid, sem_in), want, mags


@functools.lru_cache(maxsize=None)
def _sem_case(R, S):
    """_sem_host with the inputs on the device: made once per (R, S), shared by the variants, never written."""
    inputs, want, mags = _sem_host(R, S)
    return tuple(t.to(DEV) for t in inputs), want, mags


@gpu
@pytest.mark.parametrize("variant", SEM_VARIANTS)
@pytest.mark.parametrize("R,S", [(1, 8), (3, 9), (5, 13), (37, 64), (2048, 8), (4099, 24)])
def test_sem_head_wgrad_exact_integers(R, S, variant):
    """nsos_sem_head_wgrad and the four operand formats of nsos_sem_head_wgrad_x3: [dW1 | db1], dW2 and db2 bit-equal to fp64.
    Ray crossings inside 8-point groups (S = 9, 13), ragged 16-point steps, both sides of the split kernels' block split."""
    (weights, g_sem, w2, hid, sem_in), want, mags = _sem_case(R, S)
    # everything summed is a multiple of 1/4 (times the split kernels' 16 for dW1): exact while 64 * sum |terms| < 2^24
    for k, m in enumerate(mags):
        assert 64.0 * float(m.max()) < EXACT, f"output {k}: the inputs do not keep the partial sums exact"
    if variant == "exact":
        call = lambda: ops.sem_head_wgrad(weights, g_sem, w2, hid, sem_in, split_fp16=False)  # noqa: E731
    elif variant == "split_f32":
        call = lambda: ops.sem_head_wgrad(weights, g_sem, w2, hid, sem_in, split_fp16=True)  # noqa: E731
    else:
        dt = torch.bfloat16 if variant == "split_bf16" else torch.float16
        h16, x16 = hid.to(dt), sem_in.to(dt)
        assert torch.equal(h16.float(), hid) and torch.equal(x16.float(), sem_in)
        if variant.endswith("tiled"):
            x16 = ops.sem_in_tiled(x16)
        call = lambda: ops.sem_head_wgrad(weights, g_sem, w2, h16, x16, split_fp16=True)  # noqa: E731
    got, again = call(), call()
    for k, (a, b, w) in enumerate(zip(got, again, want)):
        wf = w.float().to(DEV)
        assert torch.equal(a, wf), f"output {k}: {int((a != wf).sum())} elements differ from fp64"
        assert torch.equal(_bits(a), _bits(b)), f"output {k}: not deterministic"


# ---- real data: every element within the worst-case bound of its accumulation -----------------------------------------------
REAL = [(32, 256, False), (128, 64, False), (128, 256, False), (256, 64, False), (256, 256, False), (256, 256, True)]


@gpu
@pytest.mark.parametrize("xdtype", list(_DT))
@pytest.mark.parametrize("M,N,split", REAL)
def test_wgrad_real_data_elementwise_bound(M, N, split, xdtype):
    """G = randn * 10^U(-3, 3) per row, X = relu(randn) * 10^U(-2, 2) per column: most elements of dW are invisible to a max-norm.
    Per element, against A = |G|^T |X| in fp64:
      exact kernel   |got - want| <= (L + 16) 2^-24 A      L = the longest per-wave run of points (planner): the worst case of fp32
                                                            accumulation over L terms; 16 for the MFMA's pair sum and the final cast;
      split kernel   ... + 2^-20 A                          hi + lo of both operands (2^-22 each) and the dropped lo.lo term.
    db likewise against sum |G|.  Derived bounds, not measurements; the measured err / bound is printed."""
    P = 3 * 4096 - 11 if split else wgrad_main_point(M, N)
    L = wgrad_x3_plan(P)["longest"] if split else wgrad_plan(M, N, P)["longest"]
    gen = torch.Generator().manual_seed(M * 7 + N)
    Gr = torch.randn(P, M, generator=gen) * 10.0 ** (6.0 * torch.rand(P, 1, generator=gen) - 3.0)
    Xr = torch.relu(torch.randn(P, N, generator=gen)) * 10.0 ** (4.0 * torch.rand(1, N, generator=gen) - 2.0)
    if split:   # a power of two brings max |G| to ~2^4, as backward.py does for the gradients it hands to the split kernels
        Gr = Gr * torch.exp2(torch.floor(torch.log2(16.0 / Gr.abs().max())))
    Gw = torch.full((P + 3, 300), float("nan"), device=DEV)
    Xw = torch.full((P + 3, N + 10), float("nan"), device=DEV, dtype=_DT[xdtype])
    Gw[:P, 7:7 + M] = Gr.to(DEV)
    Xw[:P, 3:3 + N] = Xr.to(DEV).to(_DT[xdtype])
    G, X = Gw[:P, 7:7 + M], Xw[:P, 3:3 + N]
    Gd, Xd = G.double(), X.double()                      # the values the kernel reads (X as stored)
    want, wantb = Gd.T @ Xd, Gd.sum(0)
    A, Ab = Gd.abs().T @ Xd, Gd.abs().sum(0)
    rel = (L + 16) * 2.0 ** -24 + (2.0 ** -20 if split else 0.0)
    Ww, bw, dW, db = _outputs(M, N)
    ops.wgrad(G, X, dW, db, split_fp16=split)
    assert _untouched(Ww, bw, M, N)
    err, errb = (dW.double() - want).abs(), (db.double() - wantb).abs()
    # db is summed from the fp32 values by both kernels: the accumulation term alone
    ratio, ratiob = float((err / (rel * A)).max()), float((errb / ((L + 16) * 2.0 ** -24 * Ab)).max())
    print(f"\nwgrad real data M={M} N={N} split={split} X={xdtype} P={P} L={L}: max err/bound dW {ratio:.4f} db {ratiob:.4f}")
    assert float(A.min()) > 0.0 and float(Ab.min()) > 0.0
    assert bool((err <= rel * A).all()), f"dW: err / bound up to {ratio:.3f}"
    assert bool((errb <= (L + 16) * 2.0 ** -24 * Ab).all()), f"db: err / bound up to {ratiob:.3f}"
