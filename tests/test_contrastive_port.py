"""CPU: the references of tests/contrastive_port.py are themselves right, and the inputs of tests/test_gpu_contrastive_edges.py
decide their picks.

* closed_form with the fp64 picks equals fp64 autograd of oracle/losses_port.nerf_contrastive (loss and gradient, 1e-12 of scale).
* sim_emulated (the kernels' fp32 arithmetic) stays within 4 x 2^-24 of the fp64 cosine matrix (measured: <= 2.4 x 2^-24).
* Every case's largest and smallest off-diagonal cosine is >= 1e-4 away from the next distinct value, and max + min > 0: no rounding
  of the order the kernels commit can move a pick or the sign under the logarithm.  No case is dropped or masked.
* The fp32 port picks the pairs the fp64 port picks (their gradients have the same non-zero rows, which are those of the fp64 picks).
* The two stress inputs meet the same input condition, and fp32 accumulation of the pair sums inside a lane -- emulated here --
  would move their matrix by >= 4 ulp ("cancel": 612 at the worst entry, 31 at the minimum) and the loss of "near_zero_sum" by
  >= 4 ulp (47), so the 1-ulp comparisons of the GPU test do separate it from the fp64 sums.
* first_extremes follows torch.argmax / argmin on sim[~eye], ties and NaN included.
"""
import numpy as np
import pytest
import torch

import contrastive_port as cp

ALL = cp.cases()
IDS = [cp.case_id(c) for c, _ in ALL]


def test_case_list_is_the_issue_s():
    assert [(c[0], c[1], c[2]) for c, _ in ALL] == [(2, 384, 3), (3, 384, 3), (4, 7, 2), (16, 63, 2), (33, 64, 2), (65, 65, 2),
                                                     (100, 257, 3), (120, 384, 3), (120, 1000, 3), (120, 5, 2)]


@pytest.mark.parametrize("case,e", ALL, ids=IDS)
def test_input_condition_gaps_and_positivity(case, e):
    gap_max, gap_min, total = cp.offdiag_gaps(cp.sim_fp64(e))
    print(f"{cp.case_id(case)}: max gap {gap_max:.3e}  min gap {gap_min:.3e}  max + min {total:.4f}")
    assert gap_max >= cp.GAP and gap_min >= cp.GAP and total > 0
    # the rows that carry gradient: one shared entry at B = 2, a shared token at B = 3, two disjoint pairs from B = 4 up
    assert len(set(cp.first_extremes(cp.sim_fp64(e)))) == min(case[0], 4)


@pytest.mark.parametrize("case,e", ALL, ids=IDS)
def test_closed_form_equals_fp64_autograd(case, e):
    picks = cp.first_extremes(cp.sim_fp64(e))
    loss, grad, mx, mn = cp.closed_form(e.double(), *picks)
    want_l, want_g = cp.port_loss_and_grad(e, torch.float64)
    assert abs(loss - want_l) <= 1e-12 * (1 + abs(want_l))
    scale = np.abs(want_g).max()
    if case[0] == 2:                                   # max and min are the same entry: loss = log 2, the gradient cancels
        assert abs(loss - np.log(2.0)) < 1e-15 and np.abs(grad).max() < 1e-15 and scale < 1e-15
        return
    assert scale > 0 and np.abs(grad - want_g).max() <= 1e-12 * scale
    rows = sorted({picks[0], picks[1], picks[2], picks[3]})
    assert len(rows) == min(case[0], 4) and sorted(np.flatnonzero(np.abs(want_g).max(-1) > 0)) == rows


@pytest.mark.parametrize("case,e", ALL, ids=IDS)
def test_emulated_similarity_is_within_the_derived_bound(case, e):
    emu, s64 = cp.sim_emulated(e), cp.sim_fp64(e)
    assert emu.dtype == np.float32 and np.array_equal(emu, emu.T)
    err = np.abs(emu.astype(np.float64) - s64).max()
    print(f"{cp.case_id(case)}: |emulated - fp64| = {err / cp.U24:.2f} x 2^-24")
    assert err <= cp.SIM_BOUND
    assert cp.first_extremes(emu) == cp.first_extremes(s64)         # "in fp32 the port picks the same pairs as in fp64"


@pytest.mark.parametrize("case,e", ALL, ids=IDS)
def test_fp32_port_picks_the_fp64_pairs(case, e):
    l32, g32 = cp.port_loss_and_grad(e, torch.float32)
    l64, g64 = cp.port_loss_and_grad(e, torch.float64)
    assert np.isfinite(l32) and abs(l32 - l64) <= cp.loss_bound(*cp.closed_form(e.double(), *cp.first_extremes(cp.sim_fp64(e)))[2:], l64)
    if case[0] == 2:
        return
    assert np.array_equal(np.abs(g32).max(-1) > 0, np.abs(g64).max(-1) > 0)
    yard = np.abs(g32 - g64).max() / np.abs(g64).max()
    print(f"{cp.case_id(case)}: fp32 port vs fp64, gradient: {yard:.2e} of scale")
    assert yard < 1e-5                                   # the same pairs: a different pick is an error of order 1


@pytest.mark.parametrize("name,e", cp.stress_cases(), ids=[n for n, _ in cp.stress_cases()])
def test_stress_inputs_decide_their_picks_and_show_fp32_accumulation(name, e):
    s64, emu, lanes = cp.sim_fp64(e), cp.sim_emulated(e), cp.sim_fp32_lanes(e)
    gap_max, gap_min, total = cp.offdiag_gaps(s64)
    picks = cp.first_extremes(s64)
    assert gap_max >= cp.GAP and gap_min >= cp.GAP and total > 0 and cp.first_extremes(emu) == picks
    assert np.abs(emu.astype(np.float64) - s64).max() <= cp.SIM_BOUND
    moved = cp.ulps(emu, lanes)
    l_emu, l_lanes = cp.loss_from_matrix(emu, picks), cp.loss_from_matrix(lanes, picks)
    print(f"{name}: max + min {total:.4f}; fp32 lanes move the matrix by <= {moved.max()} ulp ({moved[picks[2], picks[3]]} at the minimum), "
          f"the loss {l_emu} by {int(cp.ulps(l_emu, l_lanes)[0])} ulp")
    if name == "cancel":
        assert moved.max() >= 4 and moved[picks[2], picks[3]] >= 4
    else:
        assert 0 < total < 0.05 and int(cp.ulps(l_emu, l_lanes)[0]) >= 4


def test_first_extremes_is_torch_argmax_on_the_off_diagonal():
    g = torch.Generator().manual_seed(7)
    for B in (2, 3, 5, 16):
        for kind in ("plain", "ties", "nan", "const"):
            s = torch.randn(B, B, generator=g)
            if kind == "ties":
                s = torch.round(s)                     # many equal values
            if kind == "const":
                s = torch.zeros(B, B)
            if kind == "nan" and B > 2:
                s[1, 2] = s[2, 0] = float("nan")
            off = s[~torch.eye(B, dtype=torch.bool)]
            cols = torch.arange(B).repeat(B, 1)[~torch.eye(B, dtype=torch.bool)]
            rows = torch.arange(B)[:, None].repeat(1, B)[~torch.eye(B, dtype=torch.bool)]
            a, b = int(torch.argmax(off)), int(torch.argmin(off))
            assert cp.first_extremes(s.numpy()) == (int(rows[a]), int(cols[a]), int(rows[b]), int(cols[b])), (B, kind)
