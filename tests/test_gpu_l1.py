"""The L1 layer on the GPU: every row of tests/l1_table.py against its truth at a pinned iteration count, w = 0 against the plain
forward bit for bit, all eight gradients through the module, a solve that stops by itself, and a memory row.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale, t32 / t64 the
truth (l1_table.solve_l1) in float32 / float64.  `side` is compared exactly; an element may differ only where the float64 truth
says it sits within the bar for z of changing its set (l1_table.excused), and at most 1 % of a problem's elements may.
tests/test_l1_table.py shows, without a GPU, that the unthresholded iterates miss every row's bar by at least 100 x.
"""
import pytest
import torch

import lqp_py_amd as L
import l1_table as LT
import term_checks as C
from term_checks import _control, dev, cus          # (the fixtures, by name)

pytestmark = pytest.mark.gpu
LAYER = (LT.TERM, L.torch_solve_box_qp_l1, L.SolveBoxQPL1)


@pytest.mark.parametrize("key", list(LT.ROWS))
def test_row_against_the_truth(dev, cus, monkeypatch, key):
    C.row_against_the_truth(LAYER, dev, cus, monkeypatch, key)


@pytest.mark.parametrize("name", LT.SAME_BITS)
def test_w_zero_is_the_plain_forward_bit_for_bit(dev, cus, monkeypatch, name):
    zero = C.zero_term_is_the_plain_forward(LAYER, dev, cus, monkeypatch, name)
    assert float(zero["side"].abs().min()) == 1.0          # (t = 0: no kink set)


@pytest.mark.parametrize("name", list(LT.GRAD_ROWS))
def test_all_eight_gradients_through_the_module(dev, cus, monkeypatch, name):
    C.gradients_through_the_module(LAYER, dev, cus, monkeypatch, name)


def test_a_solve_that_stops_by_itself_takes_the_truths_iterations(dev):
    C.stopped_solve_takes_the_truths_iterations(LAYER, dev)


def test_no_result_depends_on_what_the_new_memory_held(dev, cus, monkeypatch):
    """In the manner of tests/mem_table.py, on tests/memharness.py: every workspace (the new regions ws, cs, t behind the forward's
    layout among them), output and temporary of a forward and a backward through the module is a guarded buffer filled with 0x00,
    then with 0xFF -- the same bits come back, no guard is touched."""
    C.no_result_depends_on_what_the_new_memory_held(LAYER, dev, cus, monkeypatch, "lqp_boxqp_forward_workspace_bytes")


def test_a_negative_or_non_finite_weight_is_refused_on_the_device(dev):
    """checked where the data are: the call that waits raises the package's ValueError and names the problem"""
    r = LT.ROWS["small_n31_m1-K10"]
    args = [None if t is None else t.to(dev) for t in LT.l1_inputs(r, 4)]
    for bad in (-1e-3, float("nan"), float("inf")):
        w = args[6].clone()
        w[2, 5, 0] = bad
        with pytest.raises(ValueError, match=r"w must be finite and >= 0, and rho positive and finite \(batch index 2\)"):
            L.torch_solve_box_qp_l1(*args[:6], w, args[7], _control(r))
    # ... and a per-problem rho: t = ws / rho is a threshold only for a positive one
    for bad in (0.0, -1.0):
        rho = torch.ones(4, 1, 1, device=dev)
        rho[1] = bad
        with pytest.raises(ValueError, match=r"rho positive and finite \(batch index 1\)"):
            L.torch_solve_box_qp_l1(*args, _control(r, rho=rho))
    sol = L.torch_solve_box_qp_l1(*args, _control(r))          # (the workspace and the layer are as good as before)
    assert sol["iter"] == r["K"] and bool(torch.isfinite(sol["x"]).all())
