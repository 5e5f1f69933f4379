"""The soft-band layer on the GPU: every row of tests/soft_table.py against its truth at a pinned iteration count, zero weights
against the plain forward and lo = hi, wl = wu against the L1 layer bit for bit, all ten gradients through the module, a solve that
stops by itself, a memory row, the refusals made on the device, sync=False.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale, t32 / t64 the
truth (soft_table.solve_soft) in float32 / float64.  `zone` is compared exactly; an element may differ only where the float64 truth
says it sits within the bar for z of changing its set (soft_table.excused), and at most 1 % of a problem's elements may.
tests/test_soft_table.py shows, without a GPU, that the iterates of the plain step and of the L1 step around the band's middle miss
every row's bar for z by at least 100 x.
"""
import pytest
import torch

import lqp_py_amd as L
import soft_table as ST
import term_checks as C
from term_checks import _control, dev, cus          # (the fixtures, by name)
import tier_table as T

pytestmark = pytest.mark.gpu
LAYER = (ST.TERM, L.torch_solve_box_qp_soft, L.SolveBoxQPSoft)


@pytest.mark.parametrize("key", list(ST.ROWS))
def test_row_against_the_truth(dev, cus, monkeypatch, key):
    C.row_against_the_truth(LAYER, dev, cus, monkeypatch, key)


@pytest.mark.parametrize("name", ST.SAME_BITS)
def test_zero_weights_are_the_plain_forward_bit_for_bit(dev, cus, monkeypatch, name):
    zero = C.zero_term_is_the_plain_forward(LAYER, dev, cus, monkeypatch, name)
    assert not bool((zero["zone"].abs() == 1).any())          # (no weight, no kink set)


@pytest.mark.parametrize("name", ST.L1EQ_ROWS)
def test_l1eq_is_the_l1_layer_bit_for_bit(dev, cus, monkeypatch, name):
    """lo = hi = c, wl = wu = w on the same device: the L1 kernels, pinned by tests/test_gpu_l1.py, are the reference"""
    r = dict(T.ROW_BY_NAME[name], soft="l1eq", l1="plain", alpha=ST.LT.ALPHA if name in ST.LT.RELAXED else 1.0)
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, B)]
    assert torch.equal(args[6], args[7]) and torch.equal(args[8], args[9])
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    l1 = L.torch_solve_box_qp_l1(*args[:6], args[6], args[8], _control(r))
    soft = L.torch_solve_box_qp_soft(*args, _control(r))
    assert l1["iter"] == soft["iter"] == r["K"]
    for k in ("loop_kind", "loop_workgroups", "linsolve_used", "mode_used", "n_factor"):
        assert l1["_stats"][k] == soft["_stats"][k], (k, l1["_stats"], soft["_stats"])
    for k in ("x", "z", "u", "u_box", "lams"):
        assert torch.equal(l1[k], soft[k]), k
    zone, side = soft["zone"], l1["side"]
    assert torch.equal(zone.abs() == 1, side == 0) and int((side == 0).sum()) > 0
    assert torch.equal(torch.where(zone.abs() == 2, zone / 2, torch.zeros_like(zone)), side)


@pytest.mark.parametrize("name", list(ST.GRAD_ROWS))
def test_all_ten_gradients_through_the_module(dev, cus, monkeypatch, name):
    _, _, g64, _, _, _ = C.gradients_through_the_module(LAYER, dev, cus, monkeypatch, name)
    for k in ("dwl", "dwu", "dlo", "dhi"):
        assert float(g64[k].abs().max()) > 0, k          # (the new gradients are not trivially zero)


def test_a_solve_that_stops_by_itself_takes_the_truths_iterations(dev):
    C.stopped_solve_takes_the_truths_iterations(LAYER, dev)


def test_no_result_depends_on_what_the_new_memory_held(dev, cus, monkeypatch):
    """In the manner of tests/mem_table.py, on tests/memharness.py: every workspace (the six new regions behind the forward's layout
    among them), output and temporary of a forward and a backward through the module is a guarded buffer filled with 0x00, then with
    0xFF -- the same bits come back, no guard is touched."""
    C.no_result_depends_on_what_the_new_memory_held(LAYER, dev, cus, monkeypatch, "lqp_boxqp_forward_l1_workspace_bytes")


MESSAGE = r"wl and wu must be finite and >= 0, lo <= hi without NaN, and rho positive and finite \(batch index %d\)"


def test_bad_band_data_are_refused_on_the_device(dev):
    """checked where the data are: the call that waits raises the package's ValueError and names the problem; the next call works"""
    r = ST.ROWS["small_n31_m1-K10"]
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, 4)]

    def solve(**over):
        a = list(args)
        for k, v in over.items():
            a[dict(wl=6, wu=7, lo=8, hi=9)[k]] = v
        return L.torch_solve_box_qp_soft(*a, _control(r))

    def planted(k, b, value):
        t = args[dict(wl=6, wu=7, lo=8, hi=9)[k]].clone()
        t[b, 5, 0] = value
        return {k: t}
    # a bad weight, on either side
    for k in ("wl", "wu"):
        for value in (-1e-3, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=MESSAGE % 2):
                solve(**planted(k, 2, value))
    # lo > hi
    with pytest.raises(ValueError, match=MESSAGE % 3):
        solve(**planted("lo", 3, float(args[9][3, 5, 0]) + 0.25))
    with pytest.raises(ValueError, match=MESSAGE % 0):
        solve(**planted("lo", 0, float("inf")))
    # NaN in lo or hi
    for k in ("lo", "hi"):
        with pytest.raises(ValueError, match=MESSAGE % 1):
            solve(**planted(k, 1, float("nan")))
    # an infinite kink on its own side is data, not an error
    ok = solve(**planted("lo", 1, -float("inf")), **planted("hi", 2, float("inf")))
    assert ok["iter"] == r["K"] and bool(torch.isfinite(ok["x"]).all())
    # a per-problem rho: tl, tu are thresholds only for a positive, finite one
    for value in (0.0, -1.0, float("inf")):
        rho = torch.ones(4, 1, 1, device=dev)
        rho[1] = value
        with pytest.raises(ValueError, match=MESSAGE % 1):
            L.torch_solve_box_qp_soft(*args, _control(r, rho=rho))
    sol = solve()          # (the workspace and the layer are as good as before)
    assert sol["iter"] == r["K"] and bool(torch.isfinite(sol["x"]).all())
