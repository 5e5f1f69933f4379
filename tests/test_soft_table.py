"""tests/soft_table.py on the CPU: the truth of the soft-band layer is solve_l1 at lo = hi, wl = wu and the oracle's loop at zero
weights, bit for bit; it satisfies the optimality conditions of the problem it claims to solve, zone by zone; its gradient recipe
matches central differences in all ten arguments; every row populates the five zones and the clamped set; a kernel that ignores the
band or takes it for an L1 term cannot pass; the Python and C entry points refuse what they cannot run.  No GPU.
"""
import ctypes
import os
import re

import pytest
import torch

import lqp_py_amd as L
import lqp_py
from lqp_py_amd import _lib
from lqp_py_amd import solve_box_qp_soft as SS
from oracle import boxqp_oracle as O
import l1_table as LT
import soft_table as ST
import term_checks as C
import tier_table as T

CUS = C.CUS
HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    return (torch.equal(a, b) if torch.is_tensor(a) else a == b)


@pytest.mark.parametrize("name", ["small_n31_m1", "sweep2_n129_m1", "lu_nonsym_n300"])
def test_zero_weights_are_the_oracle_bit_for_bit(name):
    r = dict(T.ROW_BY_NAME[name], soft="plain", l1="plain", alpha=1.0, K=30)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in ST.soft_inputs(r, 3)]
        ctl = O.make_control(**T.control(r))
        ref = O.solve_box_qp(*inp[:6], ctl)
        zero = torch.zeros_like(inp[6])
        got = ST.solve_soft(*inp[:6], zero, zero, inp[8], inp[9], ctl)
        for k in ("x", "z", "u", "rho", "iter"):
            assert _same(ref[k], got[k]), (name, dt, k)
        assert not bool((got["zone"].abs() == 1).any())          # (no weight, no kink set)


@pytest.mark.parametrize("name,alpha", [("small_n31_m1", 1.0), ("sweep2_n129_m1", LT.ALPHA), ("lu1_n300_f64", 1.0)])
def test_l1eq_is_solve_l1_bit_for_bit(name, alpha):
    """lo = hi = c, wl = wu = w: x, z, u, u_box and the iteration count of l1_table.solve_l1, over-relaxed too; zone +-1 is side 0,
    zone +-2 is side +-1"""
    r = dict(T.ROW_BY_NAME[name], soft="l1eq", l1="plain", alpha=alpha, K=60)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in ST.soft_inputs(r, 3)]
        assert torch.equal(inp[8], inp[9]) and torch.equal(inp[6], inp[7])
        ctl = O.make_control(**T.control(r))
        ref = LT.solve_l1(*inp[:6], inp[6], inp[8], ctl, alpha=alpha)
        got = ST.solve_soft(*inp, ctl, alpha=alpha)
        for k in ("x", "z", "u", "u_box", "rho", "iter", "lams"):
            assert _same(ref[k], got[k]), (name, dt, k)
        assert torch.equal((got["zone"].abs() == 1), ref["side"] == 0)
        assert torch.equal(torch.where(got["zone"].abs() == 2, got["zone"] / 2, torch.zeros_like(got["zone"])), ref["side"])
        assert int((ref["side"] == 0).sum()) > 0


def test_the_truth_satisfies_the_optimality_conditions():
    """float64 to eps = 1e-10, zone by zone: with g = Qx + p + A'nu, the band's subgradient is -wl below lo, [-wl, 0] on lo, 0 inside,
    [0, wu] on hi, wu above; off the hard bounds g + (that) = 0, on them the residual has the bound's sign and is lams"""
    r = dict(ST.ROWS["hibound_n31-K60"])
    Q, p, A, b, lb, ub, wl, wu, lo, hi = ST.soft_inputs(dict(r, dtype="f64"), 3)
    sol = ST.solve_soft(Q, p, A, b, lb, ub, wl, wu, lo, hi, O.make_control(eps_abs=1e-10, eps_rel=1e-10, max_iters=40000))
    assert sol["iter"] < 39999
    x, zone, n = sol["x"], sol["zone"], 31
    g = Q @ x + p + A.transpose(1, 2) @ sol["nus"]
    s = ST.sets(sol)
    tol = 1e-7
    assert float((A @ x - b).abs().max()) < tol and float((x - sol["z"]).abs().max()) < tol
    assert all(int(v.sum()) for v in s.values()), {k: int(v.sum()) for k, v in s.items()}
    assert float((g + wu)[s["z2"]].abs().max()) < tol and float((x - hi)[s["z2"]].min()) > -tol
    assert float((g - wl)[s["z-2"]].abs().max()) < tol and float((lo - x)[s["z-2"]].min()) > -tol
    assert float(g[s["z0"]].abs().max()) < tol
    assert float((x - lo)[s["z0"]].min()) > -tol and float((hi - x)[s["z0"]].min()) > -tol
    assert float((x - hi)[s["z1"]].abs().max()) < tol and float(g[s["z1"]].max()) < tol and float((g + wu)[s["z1"]].min()) > -tol
    assert float((x - lo)[s["z-1"]].abs().max()) < tol and float(g[s["z-1"]].min()) > -tol and float((g - wl)[s["z-1"]].max()) < tol
    # clamped: x on the bound; the band's multiplier is the rest of u, inside [-wl, wu]; the bound's has the right sign and is lams
    cl = s["clamped"]
    at_lb, at_ub = cl & (sol["u_box"] < 0), cl & (sol["u_box"] > 0)
    assert float((x - lb)[at_lb].abs().max()) < tol and float((x - ub)[at_ub].abs().max()) < tol
    band = sol["rho"] * (sol["u"] - sol["u_box"])
    assert float((band - wu).max()) < tol and float((band + wl).min()) > -tol
    res = g + band
    assert float(res[at_lb].min()) > -tol and float(res[at_ub].max()) < tol
    assert float((res - sol["lams"][:, :n] + sol["lams"][:, n:])[cl].abs().max()) < 1e-6
    # ... and everywhere: the band's multiplier is the subgradient the zone says
    assert float((band - wu)[zone == 2].abs().max()) < tol and float((band + wl)[zone == -2].abs().max()) < tol
    assert float(band[zone == 0].abs().max()) < tol


def _fd_case(seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    n, B = 12, 1
    G = rn(B, 16, n)
    Q = G.transpose(1, 2) @ G / 16 + 0.3 * torch.eye(n, dtype=torch.float64)
    p = rn(B, n, 1)
    A = rn(B, 1, n)
    lb, ub = -(0.5 + 0.6 * ru(B, n, 1)), 0.5 + 0.6 * ru(B, n, 1)
    b = A @ (0.2 * rn(B, n, 1))
    wl, wu = 0.05 + 0.6 * ru(B, n, 1), 0.05 + 0.6 * ru(B, n, 1)
    c = 0.3 * rn(B, n, 1)
    lo, hi = c - 0.3 * ru(B, n, 1), c + 0.3 * ru(B, n, 1)
    return [Q, p, A, b, lb, ub, wl, wu, lo, hi], rn(B, n, 1)


FD_SEED = 0          # (the first seed at which all six sets are populated and no element is within 2e-3 of changing sets)


def test_the_gradient_recipe_matches_central_differences():
    """n = 12, m = 1: d(cot' x*) / d(every entry of the ten arguments) by central differences of the truth run to 1e-13"""
    args, cot = _fd_case(FD_SEED)
    ctl = O.make_control(eps_abs=1e-13, eps_rel=1e-13, max_iters=100000, scale=False, adaptive_rho=False, rho=1.0)
    sol = ST.solve_soft(*args, ctl)
    sizes = {k: int(v.sum()) for k, v in ST.sets(sol).items()}
    assert all(v >= 1 for v in sizes.values()), sizes
    assert float(sol["margin"].min()) > 1e-3          # (no element near a change of set: the differences below stay on one piece)
    got = C.central_differences(ST.TERM, args, cot, ctl, sol)
    for name in ("dwl", "dwu", "dlo", "dhi"):
        assert float(got[name].abs().max()) > 1e-3, name          # (the new gradients are not trivially zero here)


@pytest.mark.parametrize("key", list(ST.ROWS))
def test_every_row_holds_the_six_sets_and_needs_the_step(key):
    # the plain iterate and the L1 iterate (c = (lo + hi) / 2, w = (wl + wu) / 2) are at least 100 bars away in z (l1eq IS the L1
    # iterate and onesided has no middle: the plain iterate alone there); the five zones (unclamped) and the clamped set
    r, idx, t32, t64, sub = C.row_needs_the_step(ST.TERM, key)
    C.row_holds_its_sets(ST.TERM, key, r, ST.sets(t64), len(idx))
    n, kind = r["n"], r["soft"]
    assert bool((sub[8] <= sub[9]).all())
    if kind == "l1eq":
        assert torch.equal(sub[8], sub[9]) and torch.equal(sub[6], sub[7])
    if kind == "onesided":
        assert bool((sub[8] == -float("inf")).all())
    if kind == "halfw":
        assert float(sub[6][:, 0::2].abs().max()) == 0.0 and float(sub[7][:, 0::2].abs().max()) == 0.0
    if kind == "hibound":
        assert int(((sub[9] == sub[5]) | (sub[8] == sub[4])).sum()) >= len(idx) * n // 5
    if kind == "allinf":
        assert bool(torch.isinf(sub[4]).all()) and bool(torch.isinf(sub[5]).all())


@pytest.mark.parametrize("name", list(ST.GRAD_ROWS))
def test_gradient_rows_have_the_same_zones_in_both_precisions(name):
    r, idx, t32, t64, sub = C.gradient_row_in_both_precisions(ST.TERM, name)
    # ... and the backward's own active set (x + u_e against the effective box) too
    act = []
    for sol, dt in ((t32, torch.float32), (t64, torch.float64)):
        lb, ub, lo, hi = (sub[k].to(dt) for k in (4, 5, 8, 9))
        K = sol["zone"].abs() == 1
        kv = torch.where(sol["zone"] == 1, hi, lo)
        wv = sol["x"] + torch.where(K, sol["u"], sol["u_box"])
        act.append((wv > torch.where(K, kv, ub)) | (wv < torch.where(K, kv, lb)))
    assert torch.equal(act[0], act[1]), name


def test_the_stopped_solve_stops_at_one_count():
    C.stopped_solve_stops_at_one_count(ST.TERM)


def test_refusals():
    n, B = 6, 2
    Q = torch.eye(n).repeat(B, 1, 1)
    p, lb, ub = torch.zeros(B, n, 1), -torch.ones(B, n, 1), torch.ones(B, n, 1)
    wl, wu, lo, hi = torch.ones(B, n, 1), torch.ones(B, n, 1), -0.1 * torch.ones(B, n, 1), 0.1 * torch.ones(B, n, 1)
    ok = L.box_qp_control()
    SS.check_soft(ok, Q, p, wl, wu, lo, hi)
    for extra in (dict(stop='each'), dict(stop='each', infeasible='flag'), dict(stop='each', unbounded='raise'), dict(unroll=True),
                  dict(backward='kkt'), dict(dist_strict_stop=True), dict(_global_bounds=(True, True)), dict(_bound_flags_dev=torch.ones(2)),
                  dict(_check_hook=lambda *a: None), dict(rho=0), dict(rho=0.0), dict(rho=-1.0)):
        for call in (lambda ctl: L.torch_solve_box_qp_soft(Q, p, None, None, lb, ub, wl, wu, lo, hi, ctl),
                     lambda ctl: L.SolveBoxQPSoft(ctl)(Q, p, None, None, lb, ub, wl, wu, lo, hi)):
            with pytest.raises(ValueError, match="lqp_py_amd"):
                call(dict(ok, **extra))
    good = (wl, wu, lo, hi)
    for k in range(4):
        for bad in (good[k][:, :3], good[k].squeeze(2), good[k].double(), None, 1.0):
            four = list(good)
            four[k] = bad
            with pytest.raises(ValueError, match="lqp_py_amd"):
                L.torch_solve_box_qp_soft(Q, p, None, None, lb, ub, *four, ok)
    # valid arguments on the CPU get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        L.torch_solve_box_qp_soft(Q, p, None, None, lb, ub, wl, wu, lo, hi, ok)
    assert lqp_py.solve_box_qp_soft.SolveBoxQPSoft is L.SolveBoxQPSoft
    assert lqp_py.solve_box_qp_soft.torch_solve_box_qp_soft is L.torch_solve_box_qp_soft


NEW_SYMBOLS = {"lqp_boxqp_forward_soft", "lqp_boxqp_forward_soft_workspace_bytes", "lqp_boxqp_soft_effective_box",
               "lqp_boxqp_soft_finish_grads"}


def test_abi_facts():
    """The new symbols are declared, exported and bound; the version is still 17; the workspace query grows by the six regions; the C
    entries refuse null pointers, the per-problem stop, the unroll factor bit, a check hook, a non-positive scalar rho and a short
    workspace before any launch -- without a GPU."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 17 and lib.lqp_abi_version() == 17
    header = open(os.path.join(os.path.dirname(HERE), "include", "lqp_amd.h")).read()
    declared = set(re.findall(r"\b(lqp_\w+)\s*\(", header))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SYMBOLS)
    for s in NEW_SYMBOLS:
        assert getattr(lib, s) is not None
    assert ctypes.sizeof(_lib.BoxQPCtrl) == lib.lqp_boxqp_ctrl_bytes() and _lib.BoxQPCtrl._fields_[-1][0] == "alpha"
    for dt, B, n, m in ((0, 4, 100, 1), (1, 3, 257, 2), (0, 2, 1025, 0)):
        fwd, l1 = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), lib.lqp_boxqp_forward_l1_workspace_bytes(dt, B, n, m)
        soft = lib.lqp_boxqp_forward_soft_workspace_bytes(dt, B, n, m)
        assert fwd + 6 * B * n * (4, 8)[dt] <= soft <= fwd + 6 * B * (n + 8) * (4, 8)[dt] + 512, (fwd, soft)
        assert soft > l1
    assert lib.lqp_boxqp_forward_soft_workspace_bytes(7, 1, 1, 0) == 0
    # refusals of the C entry (nothing is dereferenced before them: 4096 stands for any non-null pointer)
    P = ctypes.c_void_p(4096)
    ctl, stats = _lib.BoxQPCtrl(max_iters=10, check_solved=1), _lib.BoxQPStats()
    nbytes = lib.lqp_boxqp_forward_soft_workspace_bytes(0, 2, 8, 0)
    some_hook = _lib.CHECK_HOOK(lambda user, stream, counters, index: 0)

    def call(wl=P, wu=P, lo=P, hi=P, zone=P, u_box=P, ws_bytes=nbytes, hook=None, **ctl_over):
        for k, v in dict(dict(reserved2=0, rho_mode=0, rho_value=0.0), **ctl_over).items():
            setattr(ctl, k, v)
        ctl.check_hook = hook if hook is not None else _lib.CHECK_HOOK()
        return lib.lqp_boxqp_forward_soft(None, 0, 2, 8, 0, P, P, None, None, P, P, wl, wu, lo, hi, ctypes.byref(ctl), None, P, P, P, P, None, P,
                                          zone, u_box, ctypes.byref(stats), P, ws_bytes)
    for kw in (dict(wl=None), dict(wu=None), dict(lo=None), dict(hi=None), dict(zone=None), dict(u_box=None), dict(reserved2=8),
               dict(reserved2=1), dict(hook=some_hook), dict(rho_mode=1, rho_value=0.0), dict(rho_mode=1, rho_value=-1.0)):
        assert call(**kw) == 1, kw
    assert call(ws_bytes=lib.lqp_boxqp_forward_workspace_bytes(0, 2, 8, 0)) == 2
    assert call(ws_bytes=lib.lqp_boxqp_forward_l1_workspace_bytes(0, 2, 8, 0)) == 2
    assert lib.lqp_boxqp_soft_effective_box(None, 0, 2, 8, None, P, P, P, P, P, P, 1, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_soft_effective_box(None, 0, 2, 8, P, P, P, P, P, P, None, 1, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_soft_effective_box(None, 0, 2, 8, P, P, P, P, P, P, P, 2, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_soft_finish_grads(None, 0, 2, 8, P, P, None, P, P, P, P, P, P, P, P) == 1
    assert lib.lqp_boxqp_soft_finish_grads(None, 0, 2, 8, P, None, P, P, P, P, P, P, P, P, P) == 1
    assert lib.lqp_boxqp_soft_finish_grads(None, 3, 2, 8, P, P, P, P, P, P, P, P, P, P, P) == 1
