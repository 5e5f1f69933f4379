"""The piecewise-linear layer on the GPU: every row of tests/pwl_table.py against its truth at a pinned iteration count, zero slopes
against the plain forward, K = 1 with slopes (-w, w) against the L1 layer and K = 2 with slopes (-wl, 0, wu) against the soft-band
layer bit for bit, a user's K < 3 against the same call padded by hand, all eight gradients through the module, a solve that stops by
itself, a memory row, the refusals made on the device, sync=False.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale, t32 / t64 the
truth (pwl_table.solve_pwl) in float32 / float64.  `piece` is compared exactly; an element may differ only where the float64 truth
says it sits within the bar for z of changing its set (pwl_table.excused), and at most 1 % of a problem's elements may.
tests/test_pwl_table.py shows, without a GPU, that the iterates of the plain step and of the band's step on the outer kinks alone miss
every row's bar for z by at least 100 x.
"""
import pytest
import torch

import lqp_py_amd as L
import l1_table as LT
import pwl_table as PT
import soft_table as ST
import term_checks as C
from term_checks import _control, _on_dev, _pick, _report, dev, cus          # (the fixtures, by name)
import tier_table as T

pytestmark = pytest.mark.gpu
LAYER = (PT.TERM, L.torch_solve_box_qp_pwl, L.SolveBoxQPPwl)


@pytest.mark.parametrize("key", list(PT.ROWS))
def test_row_against_the_truth(dev, cus, monkeypatch, key):
    C.row_against_the_truth(LAYER, dev, cus, monkeypatch, key)


@pytest.mark.parametrize("name", PT.SAME_BITS)
def test_zero_slopes_are_the_plain_forward_bit_for_bit(dev, cus, monkeypatch, name):
    zero = C.zero_term_is_the_plain_forward(LAYER, dev, cus, monkeypatch, name)
    assert not bool((zero["piece"] % 2 == 1).any())          # (no jump, no kink set)


def _same_solve(a, b, keys=("x", "z", "u", "u_box", "lams")):
    for k in ("loop_kind", "loop_workgroups", "linsolve_used", "mode_used", "n_factor"):
        assert a["_stats"][k] == b["_stats"][k], (k, a["_stats"], b["_stats"])
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", PT.EQ_ROWS)
def test_l1eq_is_the_l1_layer_bit_for_bit(dev, cus, monkeypatch, name):
    """the user's K = 1, slopes (-w, w), on the same device: the L1 kernels, pinned by tests/test_gpu_l1.py, are the reference; and
    the same call padded by hand to three kinks"""
    r = dict(T.ROW_BY_NAME[name], pwl="l1eq", soft="plain", l1="plain", alpha=LT.ALPHA if name in LT.RELAXED else 1.0)
    B = T.batch(r, cus)
    args = _on_dev(PT.pwl_inputs(r, B), dev)
    l1a = _on_dev(LT.l1_inputs(r, B), dev)
    assert args[7].shape[2] == 1 and torch.equal(args[6][:, :, 1:], l1a[6]) and torch.equal(args[7], l1a[7])
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    l1 = L.torch_solve_box_qp_l1(*l1a, _control(r))
    pwl = L.torch_solve_box_qp_pwl(*args, _control(r))
    assert l1["iter"] == pwl["iter"] == r["K"]
    _same_solve(l1, pwl)
    assert torch.equal(pwl["piece"] - 1, l1["side"]) and int((l1["side"] == 0).sum()) > 0
    byhand = L.torch_solve_box_qp_pwl(*args[:6], *PT.pad(args[6], args[7]), _control(r))
    _same_solve(pwl, byhand, keys=("x", "z", "u", "u_box", "lams", "piece"))


@pytest.mark.parametrize("name", PT.EQ_ROWS)
def test_bandeq_is_the_soft_layer_bit_for_bit(dev, cus, monkeypatch, name):
    """the user's K = 2, slopes (-wl, 0, wu): the soft-band kernels, pinned by tests/test_gpu_soft.py, are the reference; and the same
    call padded by hand to three kinks"""
    r = dict(T.ROW_BY_NAME[name], pwl="bandeq", soft="plain", l1="plain", alpha=LT.ALPHA if name in LT.RELAXED else 1.0)
    B = T.batch(r, cus)
    args = _on_dev(PT.pwl_inputs(r, B), dev)
    sa = _on_dev(ST.soft_inputs(r, B), dev)
    assert args[7].shape[2] == 2 and torch.equal(args[7], torch.cat((sa[8], sa[9]), 2))
    assert torch.equal(args[6], torch.cat((-sa[6], 0 * sa[6], sa[7]), 2))
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    soft = L.torch_solve_box_qp_soft(*sa, _control(r))
    pwl = L.torch_solve_box_qp_pwl(*args, _control(r))
    assert soft["iter"] == pwl["iter"] == r["K"]
    _same_solve(soft, pwl)
    assert torch.equal(pwl["piece"] - 2, soft["zone"]) and all(int((soft["zone"] == k).sum()) > 0 for k in ST.ZONES)
    byhand = L.torch_solve_box_qp_pwl(*args[:6], *PT.pad(args[6], args[7]), _control(r))
    _same_solve(pwl, byhand, keys=("x", "z", "u", "u_box", "lams", "piece"))


@pytest.mark.parametrize("name", list(PT.GRAD_ROWS))
def test_all_eight_gradients_through_the_module(dev, cus, monkeypatch, name):
    _, hip, g64, _, _, _ = C.gradients_through_the_module(LAYER, dev, cus, monkeypatch, name)
    for k in range(4):
        assert float(g64["ds"][:, :, k].abs().max()) > 0 and float(hip["ds"][:, :, k].abs().max()) > 0, k      # (not trivially zero, in every slot)
    for k in range(3):
        assert float(g64["dc"][:, :, k].abs().max()) > 0 and float(hip["dc"][:, :, k].abs().max()) > 0, k


def test_gradients_of_a_users_two_kinks_have_the_users_shapes(dev, cus):
    """K = 2 through the module: ds (B, n, 3) and dc (B, n, 2), the slots the caller gave -- against the truth's recipe at K = 2"""
    r = dict(PT.GRAD_ROWS["lu1_n300_f64"], pwl="bandeq")
    B = T.batch(r, cus)
    idx = T.sample(B)
    args = _on_dev(PT.pwl_inputs(r, B), dev)
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in args]
    cot = PT.cot_of(r, B, args[1].dtype)
    x = L.SolveBoxQPPwl(control=_control(r))(*leaves)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    sub = PT.pwl_inputs(r, B, idx)
    t64 = PT.truth(r, sub, torch.float64)
    g64 = PT.truth_grads(r, sub, t64, cot[idx], torch.float64)
    assert leaves[6].grad.shape == args[6].shape == (B, r["n"], 3) and leaves[7].grad.shape == args[7].shape == (B, r["n"], 2)
    res = T.compare(r, {"ds": _pick(leaves[6].grad, idx), "dc": _pick(leaves[7].grad, idx)}, None, g64, keys=("ds", "dc"))
    _report("K=2", res)
    assert all(rec["ok"] for rec in res.values()), res


def test_a_solve_that_stops_by_itself_takes_the_truths_iterations(dev):
    C.stopped_solve_takes_the_truths_iterations(LAYER, dev)


def test_no_result_depends_on_what_the_new_memory_held(dev, cus, monkeypatch):
    """In the manner of tests/mem_table.py, on tests/memharness.py: every workspace (the eleven new regions behind the forward's
    layout among them), output and temporary of a forward and a backward through the module is a guarded buffer filled with 0x00,
    then with 0xFF -- the same bits come back, no guard is touched."""
    C.no_result_depends_on_what_the_new_memory_held(LAYER, dev, cus, monkeypatch, "lqp_boxqp_forward_soft_workspace_bytes")


MESSAGE = r"s must be finite and non-decreasing, c non-decreasing without NaN, and rho positive and finite \(batch index %d\)"


def test_bad_term_data_are_refused_on_the_device(dev):
    """checked where the data are: the call that waits raises the package's ValueError and names the problem; the next call works"""
    r = PT.ROWS["small_n31_m1-K10"]
    args = _on_dev(PT.pwl_inputs(r, 4), dev)

    def solve(s=None, c=None):
        return L.torch_solve_box_qp_pwl(*args[:6], args[6] if s is None else s, args[7] if c is None else c, _control(r))

    def planted(which, b, k, value):
        t = args[6 if which == "s" else 7].clone()
        t[b, 5, k] = value
        return {which: t}
    # a slope that is not finite, in every slot
    for k in range(4):
        for value in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match=MESSAGE % 2):
                solve(**planted("s", 2, k, value))
    # decreasing slopes
    with pytest.raises(ValueError, match=MESSAGE % 3):
        solve(**planted("s", 3, 1, float(args[6][3, 5, 0]) - 0.25))
    with pytest.raises(ValueError, match=MESSAGE % 0):
        solve(**planted("s", 0, 3, float(args[6][0, 5, 2]) - 1e-3))
    # decreasing kinks
    with pytest.raises(ValueError, match=MESSAGE % 3):
        solve(**planted("c", 3, 0, float(args[7][3, 5, 1]) + 0.25))
    with pytest.raises(ValueError, match=MESSAGE % 0):
        solve(**planted("c", 0, 1, float("inf")))
    # a NaN kink, in every slot
    for k in range(3):
        with pytest.raises(ValueError, match=MESSAGE % 1):
            solve(**planted("c", 1, k, float("nan")))
    # ... and through a user's K = 1, whose padding the library makes
    s1, c1 = args[6][:, :, 1:3].clone(), args[7][:, :, 1:2].clone()
    assert solve(s=s1, c=c1)["iter"] == r["K"]
    c1[2, 7, 0] = float("nan")
    with pytest.raises(ValueError, match=MESSAGE % 2):
        solve(s=s1, c=c1)
    # infinite kinks on their own side are data, not an error
    c = args[7].clone()
    c[1, 5, 0], c[2, 5, 2], c[3, 6, :] = -float("inf"), float("inf"), torch.tensor([-float("inf"), 0.0, float("inf")], device=dev)
    c[0, 4, 1:] = float("inf")
    ok = solve(c=c)
    assert ok["iter"] == r["K"] and bool(torch.isfinite(ok["x"]).all()) and bool(torch.isfinite(ok["piece"]).all())
    # a per-problem rho: the t_k are thresholds only for a positive, finite one
    for value in (0.0, -1.0, float("inf")):
        rho = torch.ones(4, 1, 1, device=dev)
        rho[1] = value
        with pytest.raises(ValueError, match=MESSAGE % 1):
            L.torch_solve_box_qp_pwl(*args, _control(r, rho=rho))
    sol = solve()          # (the workspace and the layer are as good as before)
    assert sol["iter"] == r["K"] and bool(torch.isfinite(sol["x"]).all())
