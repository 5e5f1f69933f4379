"""tests/log_table.py on the CPU: the truth of the log-barrier layer is the oracle's loop at zero weights, bit for bit; it satisfies
the optimality conditions of the problem it claims to solve, for every kind; its gradient recipe matches central differences in all
seven arguments; the step's branch form holds its precision in float32; every row populates its sets and takes the float32 truth
to the float64 truth's clamped set; a kernel that ignores the barrier cannot pass; the Python and C entry points refuse what they
cannot run.  No GPU.
"""
import ctypes
import os
import re

import pytest
import torch

import lqp_py_amd as L
import lqp_py
from lqp_py_amd import _lib
from lqp_py_amd import solve_box_qp_log as SL
from oracle import boxqp_oracle as O
import log_table as G
import term_checks as C
import tier_table as T

CUS = C.CUS
HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    return (torch.equal(a, b) if torch.is_tensor(a) else a == b)


@pytest.mark.parametrize("name", ["small_n31_m1", "sweep2_n129_m1", "lu_nonsym_n300"])
def test_zero_weights_are_the_oracle_bit_for_bit(name):
    r = dict(T.ROW_BY_NAME[name], log="plain", l1="plain", alpha=1.0, K=30)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in G.log_inputs(r, 3)]
        ctl = O.make_control(**T.control(r))
        ref = O.solve_box_qp(*inp[:6], ctl)
        got = G.solve_log(*inp[:6], torch.zeros_like(inp[6]), ctl)
        for k in ("x", "z", "u", "rho", "iter"):
            assert _same(ref[k], got[k]), (name, dt, k)
        assert not bool(got["curv"].any())


@pytest.mark.parametrize("key", ["sweep2_n129_m1-K60", "halfw_n330-K60", "poslb_n31-K60", "tiny_n330-K60", "allinf_n129-K60"])
def test_the_truth_satisfies_the_optimality_conditions(key):
    """float64 to eps = 1e-10, every kind: with g = Qx + p + A'nu - w / x, g = 0 off the hard bounds; on them g has the bound's
    sign and is lams (built from u_box); A x = b, lb <= x <= ub, and x > 0 wherever w > 0"""
    r = dict(G.ROWS[key])
    Q, p, A, b, lb, ub, w = G.log_inputs(dict(r, dtype="f64"), 2)
    sol = G.solve_log(Q, p, A, b, lb, ub, w, O.make_control(eps_abs=1e-10, eps_rel=1e-10, max_iters=60000))
    assert sol["iter"] < 59999
    x, n = sol["z"], r["n"]
    tol = 1e-6
    assert float((x - sol["x"]).abs().max()) < tol
    if A is not None:
        assert float((A @ sol["x"] - b).abs().max()) < tol
    assert float((lb - x).max()) <= 1e-12 and float((x - ub).max()) <= 1e-12          # (z = D zs: one rounding)
    bar = w > 0
    assert float(x[bar].min()) > 0
    xs = torch.where(bar, x, torch.ones_like(x))
    g = Q @ x + p - w / xs
    if A is not None:
        g = g + A.transpose(1, 2) @ sol["nus"]
    lam = sol["lams"][:, n:] - sol["lams"][:, :n]
    res = float((g + lam).abs().max())
    print(key, "stationarity %.2e" % res)
    assert res < tol * max(1.0, float(g.abs().max()))
    cl = sol["u_box"] != 0
    assert float(g[~cl].abs().max()) < tol
    if r["log"] != "allinf":
        at_lb, at_ub = cl & (sol["u_box"] < 0), cl & (sol["u_box"] > 0)
        assert int(at_ub.sum()) > 0 and float((x - ub)[at_ub].abs().max()) <= 1e-12 and float(g[at_ub].max()) < tol
        if int(at_lb.sum()):
            assert float((x - lb)[at_lb].abs().max()) <= 1e-12 and float(g[at_lb].min()) > -tol
        if r["log"] == "poslb":
            assert int((at_lb & bar).sum()) > 0          # (barrier elements rest on a lower bound)
    else:
        assert not bool(cl.any())
    assert torch.equal(sol["curv"] != 0, bar & ~cl)


def _fd_case(seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    n, B = 12, 2
    Gm = rn(B, 16, n)
    Q = Gm.transpose(1, 2) @ Gm / 16 + 0.3 * torch.eye(n, dtype=torch.float64)
    p = rn(B, n, 1)
    A = rn(B, 1, n)
    lb, ub = -(0.2 + 0.6 * ru(B, n, 1)), 0.2 + 0.6 * ru(B, n, 1)
    b = A @ (0.2 * ru(B, n, 1))
    w = 0.05 + 0.4 * ru(B, n, 1)
    w[:, 0::3] = 0.0
    lb[:, 1::4] = 0.05 + 0.3 * ru(B, n, 1)[:, 1::4]
    return [Q, p, A, b, lb, ub, w], rn(B, n, 1)


FD_SEED = 0          # (the first seed at which all four sets are populated and no element is within 1e-3 of changing sets)


def test_the_gradient_recipe_matches_central_differences():
    """n = 12, m = 1, two problems: d(cot' x*) / d(every entry of the seven arguments) by central differences of the truth run to
    1e-13; the entries of w that are zero are left out (dw = 0 there by convention: the one-sided derivative is another matter)"""
    args, cot = _fd_case(FD_SEED)
    ctl = O.make_control(eps_abs=1e-13, eps_rel=1e-13, max_iters=200000, scale=False, adaptive_rho=False, rho=1.0)
    sol = G.solve_log(*args, ctl)
    sizes = {k: int(v.sum()) for k, v in G.sets(sol, args[6]).items()}
    print(sizes)
    assert all(v >= 1 for v in sizes.values()), sizes
    assert float(sol["margin"].min()) > 1e-3          # (no element near a change of set: the differences below stay on one piece)
    ref = C.central_differences(G.TERM, args, cot, ctl, sol, leave_out={"dw": args[6] == 0})["dw"]
    assert float(ref.abs().max()) > 1e-3 and float(ref[args[6] == 0].abs().max()) == 0.0


def test_the_branch_form_of_the_step_holds_its_precision_in_float32():
    """prox in float32 against float64 over a grid of (v, t) with v << 0: the relative error stays at a few ulps (the form
    0.5 (v + s) would lose every digit there), S > 0 and S - t / S = v"""
    v = torch.cat((-torch.logspace(-3, 3, 61, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.logspace(-3, 3, 61, dtype=torch.float64)))
    t = torch.logspace(-6, 2, 33, dtype=torch.float64)
    V, Tt = (a.reshape(-1) for a in torch.meshgrid(v, t, indexing="ij"))
    V32, T32 = V.float(), Tt.float()
    s64 = G.prox(V32.double(), T32.double())
    s32 = G.prox(V32, T32)
    rel = ((s32.double() - s64) / s64).abs()
    print("max relative error %.2e" % float(rel.max()))
    assert float(s64.min()) > 0 and float(rel.max()) < 4e-7
    v64 = V32.double()          # (the optimality condition of the prox, S - t / S = v, in the form that does not cancel)
    assert float(((s64 - T32.double() / s64 - v64).abs() / torch.maximum(v64.abs(), s64)).max()) < 1e-12
    naive = 0.5 * (V32 + torch.sqrt(V32 * V32 + 4 * T32))
    assert float(((naive.double() - s64) / s64).abs().max()) > 1e-2          # (what the branch is for)
    assert torch.equal(G.prox(V32, torch.zeros_like(V32)), V32)


@pytest.mark.parametrize("key", list(G.ROWS))
def test_every_row_holds_its_sets_and_needs_the_step(key):
    # (the plain iterate is at least 100 bars away in z: a kernel without the step cannot pass)
    r, idx, t32, t64, sub = C.row_needs_the_step(G.TERM, key)
    n, kind = r["n"], r["log"]
    w = sub[6].double()
    assert bool((w >= 0).all()) and bool((sub[5][w > 0] > 0).all())
    C.row_holds_its_sets(G.TERM, key, r, G.sets(t64, w), len(idx))
    assert float(t64["z"][w > 0].min()) > 0
    if kind == "halfw":
        assert float(w[:, 0::2].abs().max()) == 0.0
    if kind == "poslb":
        lbp = (sub[4] > 0) & (w > 0)
        assert int(lbp.sum()) >= len(idx) * int((w[0] > 0).sum()) // 6
        assert int((lbp & (t64["u_box"] < 0)).sum()) > 0          # (barrier elements rest on a lower bound)
    if kind == "allinf":
        assert bool(torch.isinf(sub[4]).all()) and bool(torch.isinf(sub[5]).all())
    if kind == "tiny":
        shares = []

        class Watched(G.LogTerm):
            def step(self, v, rho):
                bar = self.w > 0
                shares.append(float((((v < 0) & bar).sum(dim=(1, 2)).double() / bar.sum(dim=(1, 2)).double()).min()))
                return super().step(v, rho)
        G.solve_log(*[None if a is None else a.double() for a in sub], O.make_control(**T.control(r)), alpha=r["alpha"], step=Watched)
        assert max(shares) >= G.SHARE, max(shares)


@pytest.mark.parametrize("name", list(G.GRAD_ROWS))
def test_gradient_rows_have_the_same_sets_in_both_precisions(name):
    r, idx, t32, t64, sub = C.gradient_row_in_both_precisions(G.TERM, name)
    assert torch.equal(t32["curv"] != 0, t64["curv"] != 0), name
    # ... and the backward's own active set (x + u_e against the box) too
    act = []
    for sol, dt in ((t32, torch.float32), (t64, torch.float64)):
        lb, ub = sub[4].to(dt), sub[5].to(dt)
        wv = sol["x"] + sol["u_box"]
        act.append((wv > ub) | (wv < lb))
    assert torch.equal(act[0], act[1]), name
    s = G.sets(t64, sub[6].double())
    assert all(int(v.sum()) >= G.SHARE * r["n"] for k in G.SETS for v in s[k])


def test_the_stopped_solve_stops_at_one_count():
    C.stopped_solve_stops_at_one_count(G.TERM)


def test_refusals():
    n, B = 6, 2
    Q = torch.eye(n).repeat(B, 1, 1)
    p, lb, ub = torch.zeros(B, n, 1), -torch.ones(B, n, 1), torch.ones(B, n, 1)
    w = torch.ones(B, n, 1)
    ok = L.box_qp_control()
    SL.check_log(ok, Q, p, w)
    for extra in (dict(stop='each'), dict(stop='each', infeasible='flag'), dict(stop='each', unbounded='raise'), dict(unroll=True),
                  dict(backward='kkt'), dict(dist_strict_stop=True), dict(_global_bounds=(True, True)), dict(_bound_flags_dev=torch.ones(2)),
                  dict(_check_hook=lambda *a: None), dict(rho=0), dict(rho=0.0), dict(rho=-1.0)):
        for call in (lambda ctl: L.torch_solve_box_qp_log(Q, p, None, None, lb, ub, w, ctl),
                     lambda ctl: L.SolveBoxQPLog(ctl)(Q, p, None, None, lb, ub, w)):
            with pytest.raises(ValueError, match="lqp_py_amd"):
                call(dict(ok, **extra))
    for bad in (w[:, :3], w.squeeze(2), w.double(), None, 1.0):
        with pytest.raises(ValueError, match="lqp_py_amd"):
            L.torch_solve_box_qp_log(Q, p, None, None, lb, ub, bad, ok)
    # valid arguments on the CPU get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        L.torch_solve_box_qp_log(Q, p, None, None, lb, ub, w, ok)
    assert lqp_py.solve_box_qp_log.SolveBoxQPLog is L.SolveBoxQPLog
    assert lqp_py.solve_box_qp_log.torch_solve_box_qp_log is L.torch_solve_box_qp_log


NEW_SYMBOLS = {"lqp_boxqp_forward_log", "lqp_boxqp_forward_log_workspace_bytes", "lqp_boxqp_backward_fp_curv",
               "lqp_boxqp_log_effective_duals", "lqp_boxqp_log_finish_grads"}


def test_abi_facts():
    """The new symbols are declared, exported and bound, and header == exports == binding over the whole interface; the version is
    still 17; the workspace query grows by the two regions; the C entries refuse null pointers, the per-problem stop, the unroll
    factor bit, a check hook, a non-positive scalar rho, a short workspace and a prefactored curvature backward before any launch --
    without a GPU."""
    import subprocess
    lib = _lib.load()
    assert _lib.ABI_VERSION == 17 and lib.lqp_abi_version() == 17
    header = open(os.path.join(os.path.dirname(HERE), "include", "lqp_amd.h")).read()
    declared = set(re.findall(r"\b(lqp_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lqp_\w+)", nm))
    assert NEW_SYMBOLS <= declared and declared == exported == set(_lib.SYMBOLS), (declared ^ exported, declared ^ set(_lib.SYMBOLS))
    for s in NEW_SYMBOLS:
        assert getattr(lib, s) is not None
    assert _lib.RP_LOG_INPUT == 1 << 20
    for dt, B, n, m in ((0, 4, 100, 1), (1, 3, 257, 2), (0, 2, 1025, 0)):
        fwd, soft = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), lib.lqp_boxqp_forward_soft_workspace_bytes(dt, B, n, m)
        lg = lib.lqp_boxqp_forward_log_workspace_bytes(dt, B, n, m)
        assert fwd + 2 * B * n * (4, 8)[dt] <= lg <= fwd + 2 * B * (n + 8) * (4, 8)[dt] + 512, (fwd, lg)
        assert lg < soft
    assert lib.lqp_boxqp_forward_log_workspace_bytes(7, 1, 1, 0) == 0
    # refusals of the C entry (nothing is dereferenced before them: 4096 stands for any non-null pointer)
    P = ctypes.c_void_p(4096)
    ctl, stats = _lib.BoxQPCtrl(max_iters=10, check_solved=1), _lib.BoxQPStats()
    nbytes = lib.lqp_boxqp_forward_log_workspace_bytes(0, 2, 8, 0)
    some_hook = _lib.CHECK_HOOK(lambda user, stream, counters, index: 0)

    def call(w=P, u_box=P, curv=P, ws_bytes=nbytes, hook=None, **ctl_over):
        for k, v in dict(dict(reserved2=0, rho_mode=0, rho_value=0.0), **ctl_over).items():
            setattr(ctl, k, v)
        ctl.check_hook = hook if hook is not None else _lib.CHECK_HOOK()
        return lib.lqp_boxqp_forward_log(None, 0, 2, 8, 0, P, P, None, None, P, P, w, ctypes.byref(ctl), None, P, P, P, P, None, P,
                                         u_box, curv, ctypes.byref(stats), P, ws_bytes)
    for kw in (dict(w=None), dict(u_box=None), dict(curv=None), dict(reserved2=8), dict(reserved2=1), dict(hook=some_hook),
               dict(rho_mode=1, rho_value=0.0), dict(rho_mode=1, rho_value=-1.0)):
        assert call(**kw) == 1, kw
    assert call(ws_bytes=lib.lqp_boxqp_forward_workspace_bytes(0, 2, 8, 0)) == 2
    assert lib.lqp_boxqp_log_effective_duals(None, 0, 2, 8, None, 1, 1.0, None, P, P) == 1
    assert lib.lqp_boxqp_log_effective_duals(None, 0, 2, 8, P, 2, 1.0, None, P, P) == 1
    assert lib.lqp_boxqp_log_effective_duals(None, 0, 2, 8, P, 3, 1.0, None, P, P) == 1
    assert lib.lqp_boxqp_log_finish_grads(None, 0, 2, 8, None, P, P, P) == 1
    assert lib.lqp_boxqp_log_finish_grads(None, 3, 2, 8, P, P, P, P) == 1
    assert lib.lqp_boxqp_log_finish_grads(None, 0, 2, 8, P, P, P, None) == 0          # (dw = NULL: nothing to do)
    fail = ctypes.c_int32(-1)
    bwd = lambda linsolve: lib.lqp_boxqp_backward_fp_curv(None, 0, 2, 8, 0, P, P, P, P, None, P, None, P, P, P, 1, 1.0, None, P, P, None, None,
                                                          P, P, ctypes.byref(fail), P, 0, linsolve, None)
    assert bwd(2 | 0x100) == 1 and bwd(1 | 0x100) == 1          # (LQP_BWD_PREFACTORED: no prefactor phase carries the diagonal)
    assert bwd(1) == 2                                          # (the next refusal in line: the workspace is too short)
