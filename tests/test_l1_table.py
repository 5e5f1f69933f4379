"""tests/l1_table.py on the CPU: the truth of the L1 layer is the oracle's loop at w = 0, satisfies the optimality conditions of the
problem it claims to solve, its gradient recipe matches central differences, every row exercises the three sets, a kernel that
ignores w cannot pass, and the Python entry points refuse what they cannot run.  No GPU.
"""
import os
import re

import numpy as np
import pytest
import torch

import lqp_py_amd as L
import lqp_py
from lqp_py_amd import _lib
from lqp_py_amd import solve_box_qp_l1 as S1
from oracle import boxqp_oracle as O
import l1_table as LT
import term_checks as C
import tier_table as T

CUS = C.CUS
HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    return (torch.equal(a, b) if torch.is_tensor(a) else a == b)


@pytest.mark.parametrize("name", ["small_n31_m1", "sweep2_n129_m1", "lu_nonsym_n300"])
def test_w_zero_is_the_oracle_bit_for_bit(name):
    r = dict(T.ROW_BY_NAME[name], l1="plain", alpha=1.0, K=30)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in LT.l1_inputs(r, 3)]
        ctl = O.make_control(**T.control(r))
        ref = O.solve_box_qp(*inp[:6], ctl)
        got = LT.solve_l1(*inp[:6], torch.zeros_like(inp[6]), inp[7], ctl)
        for k in ("x", "z", "u", "rho", "iter"):
            assert _same(ref[k], got[k]), (name, dt, k)
        assert float(got["side"].abs().min()) == 1.0          # (t = 0: no kink set)


def test_w_zero_is_the_oracle_on_golden_g1():
    g = np.load(os.path.join(HERE, "golden", "g1_b32_n10_box.npz"), allow_pickle=True)
    Q, p, lb, ub = (torch.tensor(g[k]) for k in ("Q", "p", "lb", "ub"))
    ctl = O.make_control(eps_abs=1e-5, eps_rel=1e-5)
    ref = O.solve_box_qp(Q, p, None, None, lb, ub, ctl)
    got = LT.solve_l1(Q, p, None, None, lb, ub, torch.zeros_like(p), torch.zeros_like(p), ctl)
    assert ref["iter"] == int(g["iter"]) > 0
    for k in ("x", "z", "u", "rho", "iter"):
        assert _same(ref[k], got[k]), k


def test_the_truth_satisfies_the_optimality_conditions():
    """float64 to eps = 1e-10: stationarity g = Qx + p + A'nu with -+w off the kink, |g| <= w on it, the sign conditions at bounds"""
    r = dict(LT.ROWS["small_n31_m1-K60"], l1="cbound")
    Q, p, A, b, lb, ub, w, c = LT.l1_inputs(dict(r, dtype="f64"), 3)
    sol = LT.solve_l1(Q, p, A, b, lb, ub, w, c, O.make_control(eps_abs=1e-10, eps_rel=1e-10, max_iters=20000))
    assert sol["iter"] < 19999
    x = sol["x"]
    g = Q @ x + p + A.transpose(1, 2) @ sol["nus"]
    kink, free, clamped = LT.sets(sol)
    tol = 1e-7
    assert float((A @ x - b).abs().max()) < tol and float((x - sol["z"]).abs().max()) < tol
    assert int(kink.sum()) and int(free.sum()) and int(clamped.sum())
    # thresholded free: g + side w = 0
    assert float((g + sol["side"] * w)[free].abs().max()) < tol
    # on the kink (inside the box, or resting on a bound that c equals): x = c; inside the box |g| <= w
    assert float((x - c)[kink].abs().max()) < tol
    inside = kink & (c > lb) & (c < ub)
    assert int(inside.sum()) and float((g.abs() - w)[inside].max()) < tol
    # clamped: x on the bound, and the multiplier of the bound has the right sign: g + side w = lam_lo - lam_hi
    at_lb, at_ub = clamped & (sol["u_box"] < 0), clamped & (sol["u_box"] > 0)
    assert float((x - lb)[at_lb].abs().max()) < tol and float((x - ub)[at_ub].abs().max()) < tol
    res = g + sol["side"] * w
    assert float(res[at_lb].min()) > -tol and float(res[at_ub].max()) < tol
    assert float((res - sol["lams"][:, :31] + sol["lams"][:, 31:])[clamped].abs().max()) < 1e-6


def test_the_gradient_recipe_matches_central_differences():
    """n = 8, m = 1: d(cot' x*) / d(every entry of the eight arguments) by central differences of the truth run to 1e-13"""
    torch.manual_seed(5)
    n, B = 8, 1
    G = torch.randn(B, 12, n, dtype=torch.float64)
    Q = G.transpose(1, 2) @ G / 12 + 0.3 * torch.eye(n, dtype=torch.float64)
    p = torch.randn(B, n, 1, dtype=torch.float64)
    A = torch.randn(B, 1, n, dtype=torch.float64)
    lb = -(0.4 + 0.6 * torch.rand(B, n, 1, dtype=torch.float64))
    ub = 0.4 + 0.6 * torch.rand(B, n, 1, dtype=torch.float64)
    b = A @ (0.2 * torch.randn(B, n, 1, dtype=torch.float64))
    w = 0.05 + 0.6 * torch.rand(B, n, 1, dtype=torch.float64)
    c = 0.3 * torch.randn(B, n, 1, dtype=torch.float64)
    cot = torch.randn(B, n, 1, dtype=torch.float64)
    ctl = O.make_control(eps_abs=1e-13, eps_rel=1e-13, max_iters=100000, scale=False, adaptive_rho=False, rho=1.0)
    args = [Q, p, A, b, lb, ub, w, c]
    sol = LT.solve_l1(*args, ctl)
    kink, free, clamped = LT.sets(sol)
    assert int(kink.sum()) >= 1 and int(free.sum()) >= 1 and int(clamped.sum()) >= 1, (kink.sum(), free.sum(), clamped.sum())
    assert float(sol["margin"].min()) > 1e-3          # (no element near a change of set: the differences below stay on one piece)
    C.central_differences(LT.TERM, args, cot, ctl, sol)


@pytest.mark.parametrize("key", list(LT.ROWS))
def test_every_row_holds_the_three_sets_and_needs_w(key):
    # (the unthresholded iterates, w = 0, are the other step here: a kernel that ignores w cannot pass)
    r, idx, t32, t64, sub = C.row_needs_the_step(LT.TERM, key)
    n = r["n"]
    for b, (k, f, c) in enumerate(zip(*LT.sets(t64))):
        sizes = (int(k.sum()), int(f.sum()), int(c.sum()))
        need = (n / 10, n / 10, 0 if r["l1"] == "allinf" else n / 10)      # (no bound, nothing clamped)
        assert all(s >= q for s, q in zip(sizes, need)), (key, b, sizes)
    if r["l1"] == "halfw":
        assert float(sub[6][:, 0::2].abs().max()) == 0.0
    if r["l1"] == "cbound":
        assert int(((sub[7] == sub[4]) | (sub[7] == sub[5])).sum()) >= len(idx) * n // 5


@pytest.mark.parametrize("name", list(LT.GRAD_ROWS))
def test_gradient_rows_have_the_same_sets_in_both_precisions(name):
    r, idx, t32, t64, sub = C.gradient_row_in_both_precisions(LT.TERM, name)
    for a, b in zip(LT.sets(t32), LT.sets(t64)):
        assert torch.equal(a, b), name
    # ... and the backward's own active set (x + u_e against the effective box) too
    act = []
    for sol, dt in ((t32, torch.float32), (t64, torch.float64)):
        lb, ub, c = (sub[k].to(dt) for k in (4, 5, 7))
        K = sol["side"] == 0
        wv = sol["x"] + torch.where(K, sol["u"], sol["u_box"])
        act.append((wv > torch.where(K, c, ub)) | (wv < torch.where(K, c, lb)))
    assert torch.equal(act[0], act[1]), name


def test_the_stopped_solve_stops_at_one_count():
    C.stopped_solve_stops_at_one_count(LT.TERM)


def test_refusals():
    n, B = 6, 2
    Q = torch.eye(n).repeat(B, 1, 1)
    p, lb, ub = torch.zeros(B, n, 1), -torch.ones(B, n, 1), torch.ones(B, n, 1)
    w, c = torch.ones(B, n, 1), torch.zeros(B, n, 1)
    ok = L.box_qp_control()
    S1.check_l1(ok, Q, p, w, c)
    for extra in (dict(stop='each'), dict(stop='each', infeasible='flag'), dict(stop='each', unbounded='raise'), dict(unroll=True),
                  dict(backward='kkt'), dict(dist_strict_stop=True), dict(_global_bounds=(True, True)), dict(_bound_flags_dev=torch.ones(2)),
                  dict(_check_hook=lambda *a: None), dict(rho=0), dict(rho=0.0)):
        for call in (lambda ctl: L.torch_solve_box_qp_l1(Q, p, None, None, lb, ub, w, c, ctl),
                     lambda ctl: L.SolveBoxQPL1(ctl)(Q, p, None, None, lb, ub, w, c)):
            with pytest.raises(ValueError, match="lqp_py_amd"):
                call(dict(ok, **extra))
    for bw, bc in ((w[:, :3], c), (w, c.squeeze(2)), (w.double(), c), (w, c.double()), (None, c), (w, 1.0)):
        with pytest.raises(ValueError, match="lqp_py_amd"):
            L.torch_solve_box_qp_l1(Q, p, None, None, lb, ub, bw, bc, ok)
    # valid arguments on the CPU get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        L.torch_solve_box_qp_l1(Q, p, None, None, lb, ub, w, c, ok)
    assert lqp_py.solve_box_qp_l1.SolveBoxQPL1 is L.SolveBoxQPL1 and lqp_py.solve_box_qp_l1.torch_solve_box_qp_l1 is L.torch_solve_box_qp_l1


NEW_SYMBOLS = {"lqp_boxqp_forward_l1", "lqp_boxqp_forward_l1_workspace_bytes", "lqp_boxqp_l1_effective_box", "lqp_boxqp_l1_finish_grads"}


def test_abi_facts():
    """The new symbols -- the forward, its workspace size and the two element-wise entries of the backward: the issue counts three,
    its own list names these four -- are declared, exported and bound; the version is still 17; the C entry refuses null pointers,
    the per-problem stop and a short workspace before any launch."""
    import ctypes
    lib = _lib.load()
    assert _lib.ABI_VERSION == 17 and lib.lqp_abi_version() == 17
    header = open(os.path.join(os.path.dirname(HERE), "include", "lqp_amd.h")).read()
    declared = set(re.findall(r"\b(lqp_\w+)\s*\(", header))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SYMBOLS)
    for s in NEW_SYMBOLS:
        assert getattr(lib, s) is not None
    assert ctypes.sizeof(_lib.BoxQPCtrl) == lib.lqp_boxqp_ctrl_bytes() and _lib.BoxQPCtrl._fields_[-1][0] == "alpha"
    for dt, B, n, m in ((0, 4, 100, 1), (1, 3, 257, 2)):
        fwd, l1 = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), lib.lqp_boxqp_forward_l1_workspace_bytes(dt, B, n, m)
        assert fwd + 3 * B * n * (4, 8)[dt] <= l1 <= fwd + 3 * B * (n + 8) * (4, 8)[dt] + 512, (fwd, l1)
    assert lib.lqp_boxqp_forward_l1_workspace_bytes(7, 1, 1, 0) == 0
    # refusals of the C entry (nothing is dereferenced before them: 4096 stands for any non-null pointer)
    P = ctypes.c_void_p(4096)
    ctl, stats = _lib.BoxQPCtrl(max_iters=10, check_solved=1), _lib.BoxQPStats()
    nbytes = lib.lqp_boxqp_forward_l1_workspace_bytes(0, 2, 8, 0)

    def call(w=P, c=P, side=P, u_box=P, ws_bytes=nbytes, **ctl_over):
        for k, v in dict(dict(reserved2=0, rho_mode=0, rho_value=0.0), **ctl_over).items():
            setattr(ctl, k, v)
        return lib.lqp_boxqp_forward_l1(None, 0, 2, 8, 0, P, P, None, None, P, P, w, c, ctypes.byref(ctl), None, P, P, P, P, None, P, side, u_box,
                                        ctypes.byref(stats), P, ws_bytes)
    for kw in (dict(w=None), dict(c=None), dict(side=None), dict(u_box=None), dict(reserved2=8), dict(reserved2=1),
               dict(rho_mode=1, rho_value=0.0)):
        assert call(**kw) == 1, kw
    assert call(ws_bytes=lib.lqp_boxqp_forward_workspace_bytes(0, 2, 8, 0)) == 2
    assert lib.lqp_boxqp_l1_effective_box(None, 0, 2, 8, None, P, P, P, P, P, 1, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_l1_finish_grads(None, 0, 2, 8, P, None, P, P, P, P, P, P) == 1
