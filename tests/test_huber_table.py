"""tests/huber_table.py on the CPU: the truth of the Huber layer is the oracle's loop at zero weights, bit for bit; with delta = +inf
everywhere it is the plain solve of (Q + diag(w), p - w c); it satisfies the optimality conditions of the problem it claims to solve,
zone by zone and for every kind; its gradient recipe matches central differences in all nine arguments; every row populates its sets
and takes the float32 truth to the float64 truth's zones; a kernel with the plain step, with the pure quadratic step or with the L1
step at weight w delta cannot pass; the Python and C entry points refuse what they cannot run.  No GPU.
"""
import ctypes
import math
import os
import re

import pytest
import torch

import lqp_py_amd as L
import lqp_py
from lqp_py_amd import _lib
from lqp_py_amd import solve_box_qp_huber as SH
from oracle import boxqp_oracle as O
import huber_table as G
import term_checks as C
import term_table as TT
import tier_table as T

CUS = C.CUS
HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    return (torch.equal(a, b) if torch.is_tensor(a) else a == b)


@pytest.mark.parametrize("name", ["small_n31_m1", "sweep2_n129_m1", "lu_nonsym_n300"])
def test_zero_weights_are_the_oracle_bit_for_bit(name):
    """... with finite, infinite and zero deltas under them: 0 * inf never reaches the iterate"""
    r = dict(T.ROW_BY_NAME[name], huber="plain", l1="plain", alpha=1.0, K=30)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in G.huber_inputs(r, 3)]
        delta = inp[8].clone()
        delta[:, 1::3] = math.inf
        delta[:, 2::3] = 0.0
        ctl = O.make_control(**T.control(r))
        ref = O.solve_box_qp(*inp[:6], ctl)
        got = G.solve_huber(*inp[:6], torch.zeros_like(inp[6]), inp[7], delta, ctl)
        for k in ("x", "z", "u", "rho", "iter"):
            assert _same(ref[k], got[k]), (name, dt, k)
        assert not bool(got["zone"].any()) and bool(torch.isfinite(got["u_box"]).all())


def test_infinite_delta_is_the_quadratic_folded_into_Q_and_p():
    """delta = +inf everywhere: w H(x - c) = 0.5 w (x - c)^2, so the solve agrees with the plain oracle solve of (Q + diag(w),
    p - w c) -- two different iterations that each stop at eps (TT.STOP, eps = 1e-5), so they agree to a multiple of eps and not to
    rounding: the bound is the 1e4 eps that test_log_table.py asks of a solve stopped at eps (eps = 1e-10 against tol = 1e-6 there).
    The same pair at that file's eps = 1e-10 is held to its 1e-6 too: the statement that separates the two problems sharply."""
    Q, p, A, b, lb, ub, w, c, delta = G.stop_inputs(torch.float64)
    inf = torch.full_like(delta, math.inf)
    Qf, pf = Q + torch.diag_embed(w[:, :, 0]), p - w * c
    for eps, iters in ((TT.STOP_CONTROL["eps_abs"], None), (1e-10, 60000)):
        ctl = O.make_control(eps_abs=eps, eps_rel=eps, **({} if iters is None else dict(max_iters=iters)))
        got = G.solve_huber(Q, p, A, b, lb, ub, w, c, inf, ctl)
        ref = O.solve_box_qp(Qf, pf, A, b, lb, ub, O.make_control(**ctl))
        assert 0 < got["iter"] < ctl["max_iters"] - 1 and 0 < ref["iter"] < ctl["max_iters"] - 1
        err = float((got["x"] - ref["x"]).abs().max())
        print("eps %.0e" % eps, "iterations", got["iter"], ref["iter"], "|x - x_folded| %.2e" % err)
        assert err < 1e4 * eps * max(1.0, float(ref["x"].abs().max())), (eps, err)
        assert not bool(got["zone"].any())          # (no linear piece anywhere)
    plain = O.solve_box_qp(Q, p, A, b, lb, ub, O.make_control(**TT.STOP_CONTROL))
    assert float((plain["x"] - ref["x"]).abs().max()) > 1e-2          # (... and the term is not a small thing here)


@pytest.mark.parametrize("key", ["sweep2_n129_m1-K60", "halfw_n330-K60", "infdelta_n330-K60", "zerodelta_n31-K60", "allinf_n129-K60"])
def test_the_truth_satisfies_the_optimality_conditions(key):
    """float64 to eps = 1e-10, every kind: with g = Qx + p + A'nu + w clip(x - c, -delta, delta), g = 0 off the hard bounds; on them
    g has the bound's sign and is lams (built from u_box); A x = b, lb <= x <= ub; and zone by zone: x - c >= delta on zone +1,
    <= -delta on zone -1, |x - c| <= delta on zone 0 where w > 0 -- on the free elements"""
    r = dict(G.ROWS[key])
    Q, p, A, b, lb, ub, w, c, delta = G.huber_inputs(dict(r, dtype="f64"), 2)
    sol = G.solve_huber(Q, p, A, b, lb, ub, w, c, delta, O.make_control(eps_abs=1e-10, eps_rel=1e-10, max_iters=60000))
    assert sol["iter"] < 59999
    x, n = sol["z"], r["n"]
    tol = 1e-6
    assert float((x - sol["x"]).abs().max()) < tol
    if A is not None:
        assert float((A @ sol["x"] - b).abs().max()) < tol
    assert float((lb - x).max()) <= 1e-12 and float((x - ub).max()) <= 1e-12          # (z = D zs: one rounding)
    d = x - c
    g = Q @ x + p + w * torch.minimum(torch.maximum(d, -delta), delta)
    if A is not None:
        g = g + A.transpose(1, 2) @ sol["nus"]
    lam = sol["lams"][:, n:] - sol["lams"][:, :n]
    res = float((g + lam).abs().max())
    print(key, "stationarity %.2e" % res)
    assert res < tol * max(1.0, float(g.abs().max()))
    cl = sol["u_box"] != 0
    assert float(g[~cl].abs().max()) < tol
    zone, on = sol["zone"], w > 0
    assert not bool(zone[~on].any())
    # (on a free element: the zone of a clamped one is the zone of v = z + u, where the step would have gone without the bound)
    free = ~cl
    assert float((d - delta)[(zone == 1) & free].min()) > -tol and float((d + delta)[(zone == -1) & free].max()) < tol
    inside = (zone == 0) & on & free
    assert float((d.abs() - delta)[inside].max()) < tol
    assert all(int(((zone == k) & on & free).sum()) > 0 for k in (-1, 0, 1))
    if r["huber"] != "allinf":
        at_lb, at_ub = cl & (sol["u_box"] < 0), cl & (sol["u_box"] > 0)
        assert int(at_ub.sum()) > 0 and float((x - ub)[at_ub].abs().max()) <= 1e-12 and float(g[at_ub].max()) < tol
        assert int(at_lb.sum()) > 0 and float((x - lb)[at_lb].abs().max()) <= 1e-12 and float(g[at_lb].min()) > -tol
        assert int((cl & on).sum()) > 0          # (the term pushes on clamped elements too: u_box is not S - clamp(S))
    else:
        assert not bool(cl.any())
    if r["huber"] == "infdelta":
        assert not bool(zone[torch.isinf(delta)].any())
    if r["huber"] == "zerodelta":
        z0 = (delta == 0) & on
        assert bool((zone[z0] != 0).any()) and float((w * torch.minimum(torch.maximum(d, -delta), delta))[z0].abs().max()) == 0.0


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
    w = 0.5 + 2.0 * ru(B, n, 1)
    w[:, 0::4] = 0.0
    c = 0.4 * rn(B, n, 1)
    delta = 0.05 + 0.3 * ru(B, n, 1)
    return [Q, p, A, b, lb, ub, w, c, delta], rn(B, n, 1)


FD_SEED = 0          # (the first seed at which all five sets are populated and no element is within 1e-3 of changing sets)


def test_the_gradient_recipe_matches_central_differences():
    """n = 12, m = 1, two problems: d(cot' x*) / d(every entry of the nine arguments) by central differences of the truth run to
    1e-13.  The term is C1 and no element sits near a change of set, so every entry has a two-sided derivative: w = 0 included
    (dw = dp clip(z - c, -delta, delta) there too)."""
    args, cot = _fd_case(FD_SEED)
    ctl = O.make_control(eps_abs=1e-13, eps_rel=1e-13, max_iters=200000, scale=False, adaptive_rho=False, rho=1.0)
    sol = G.solve_huber(*args, ctl)
    sizes = {k: int(v.sum()) for k, v in G.sets(sol, args[6]).items()}
    print(sizes)
    assert all(v >= 1 for v in sizes.values()), sizes
    assert float(sol["margin"].min()) > 1e-3          # (no element near a change of set: the differences below stay on one piece)
    got = C.central_differences(G.TERM, args, cot, ctl, sol)
    assert all(float(got[k].abs().max()) > 1e-3 for k in ("dw", "dc", "ddelta"))


@pytest.mark.parametrize("key", list(G.ROWS))
def test_every_row_holds_its_sets_and_needs_the_step(key):
    # (the plain, the pure quadratic and the L1 iterate are at least 100 bars away in z: a kernel that lost a branch cannot pass)
    r, idx, t32, t64, sub = C.row_needs_the_step(G.TERM, key)
    assert set(G.TERM.steps_of(r["huber"])) == {"plain", "quadratic", "l1"}
    kind = r["huber"]
    w, c, delta = (t.double() for t in sub[6:9])
    assert bool((w >= 0).all()) and bool((delta >= 0).all()) and bool(torch.isfinite(c).all())
    C.row_holds_its_sets(G.TERM, key, r, G.sets(t64, w), len(idx))
    if kind == "halfw":
        assert float(w[:, 0::2].abs().max()) == 0.0
    if kind == "infdelta":
        assert bool(torch.isinf(delta[:, 1::3]).all()) and not bool(t64["zone"][:, 1::3].any())
    if kind == "zerodelta":
        assert float(delta[:, 1::3].abs().max()) == 0.0
    if kind == "allinf":
        assert bool(torch.isinf(sub[4]).all()) and bool(torch.isinf(sub[5]).all())


@pytest.mark.parametrize("name", list(G.GRAD_ROWS))
def test_gradient_rows_have_the_same_sets_in_both_precisions(name):
    r, idx, t32, t64, sub = C.gradient_row_in_both_precisions(G.TERM, name)
    w = sub[6].double()
    assert torch.equal(G.curv_of(t32, sub[6].float()) != 0, G.curv_of(t64, w) != 0), name
    # no sampled element lies within the bar for z of a zone boundary: curv jumps there
    zbar = T.compare(r, {"z": t32["z"]}, t32 if r["dtype"] == "f32" else None, t64, keys=("z",))["z"]["bar"]
    print(name, "nearest zone boundary %.2e" % float(t64["zmargin"].min()), "bar for z %.2e" % zbar)
    assert float(t64["zmargin"].min()) > zbar, name
    # ... and the backward's own active set (x + u_e against the box) is the same too
    act = []
    for sol, dt in ((t32, torch.float32), (t64, torch.float64)):
        lb, ub = sub[4].to(dt), sub[5].to(dt)
        wv = sol["x"] + sol["u_box"]
        act.append((wv > ub) | (wv < lb))
    assert torch.equal(act[0], act[1]), name
    s = G.sets(t64, w)
    assert all(int(v.sum()) >= G.SHARE * r["n"] for k in G.SETS for v in s[k])


def test_the_stopped_solve_stops_at_one_count():
    C.stopped_solve_stops_at_one_count(G.TERM)


def test_refusals():
    n, B = 6, 2
    Q = torch.eye(n).repeat(B, 1, 1)
    p, lb, ub = torch.zeros(B, n, 1), -torch.ones(B, n, 1), torch.ones(B, n, 1)
    w, c, delta = torch.ones(B, n, 1), torch.zeros(B, n, 1), torch.full((B, n, 1), 0.1)
    ok = L.box_qp_control()
    SH.check_huber(ok, Q, p, w, c, delta)
    for extra in (dict(stop='each'), dict(stop='each', infeasible='flag'), dict(stop='each', unbounded='raise'), dict(unroll=True),
                  dict(backward='kkt'), dict(dist_strict_stop=True), dict(_global_bounds=(True, True)), dict(_bound_flags_dev=torch.ones(2)),
                  dict(_check_hook=lambda *a: None), dict(rho=0), dict(rho=0.0), dict(rho=-1.0)):
        for call in (lambda ctl: L.torch_solve_box_qp_huber(Q, p, None, None, lb, ub, w, c, delta, ctl),
                     lambda ctl: L.SolveBoxQPHuber(ctl)(Q, p, None, None, lb, ub, w, c, delta)):
            with pytest.raises(ValueError, match="lqp_py_amd"):
                call(dict(ok, **extra))
    for bad in (w[:, :3], w.squeeze(2), w.double(), None, 1.0):
        for k in range(3):
            a = [w, c, delta]
            a[k] = bad
            with pytest.raises(ValueError, match="lqp_py_amd"):
                L.torch_solve_box_qp_huber(Q, p, None, None, lb, ub, *a, ok)
    # valid arguments on the CPU get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        L.torch_solve_box_qp_huber(Q, p, None, None, lb, ub, w, c, delta, ok)
    assert lqp_py.solve_box_qp_huber.SolveBoxQPHuber is L.SolveBoxQPHuber
    assert lqp_py.solve_box_qp_huber.torch_solve_box_qp_huber is L.torch_solve_box_qp_huber


NEW_SYMBOLS = {"lqp_boxqp_forward_huber", "lqp_boxqp_forward_huber_workspace_bytes", "lqp_boxqp_huber_effective_duals",
               "lqp_boxqp_huber_finish_grads"}


def test_abi_facts():
    """The four new symbols are declared, exported and bound, and header == exports == binding over the whole interface; the version
    is still 17; RP_HUBER_INPUT is bit 22 on both sides; the workspace query grows by the six regions; the C entries refuse null
    pointers, the per-problem stop, the unroll factor bit, a check hook, a non-positive scalar rho and a short workspace before any
    launch -- without a GPU."""
    import subprocess
    lib = _lib.load()
    assert _lib.ABI_VERSION == 17 and lib.lqp_abi_version() == 17
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "lqp_amd.h")).read()
    assert re.search(r"#define\s+LQP_ABI_VERSION\s+17\b", header)
    declared = set(re.findall(r"\b(lqp_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lqp_\w+)", nm))
    assert NEW_SYMBOLS <= declared and declared == exported == set(_lib.SYMBOLS), (declared ^ exported, declared ^ set(_lib.SYMBOLS))
    for s in NEW_SYMBOLS:
        assert getattr(lib, s) is not None
    assert _lib.RP_HUBER_INPUT == 1 << 22
    device = open(os.path.join(root, "lqp_py_amd", "csrc", "lqp_boxqp.hpp")).read()
    assert re.search(r"RP_HUBER_INPUT\s*=\s*1\s*<<\s*22\b", device)
    assert "bit 22 (4194304)" in header
    for dt, B, n, m in ((0, 4, 100, 1), (1, 3, 257, 2), (0, 2, 1025, 0)):
        fwd, soft = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), lib.lqp_boxqp_forward_soft_workspace_bytes(dt, B, n, m)
        hb = lib.lqp_boxqp_forward_huber_workspace_bytes(dt, B, n, m)
        assert fwd + 6 * B * n * (4, 8)[dt] <= hb <= fwd + 6 * B * (n + 8) * (4, 8)[dt] + 512, (fwd, hb)
        assert hb == soft          # (six regions, as the soft band has)
    assert lib.lqp_boxqp_forward_huber_workspace_bytes(7, 1, 1, 0) == 0
    # refusals of the C entry (nothing is dereferenced before them: 4096 stands for any non-null pointer)
    P = ctypes.c_void_p(4096)
    ctl, stats = _lib.BoxQPCtrl(max_iters=10, check_solved=1), _lib.BoxQPStats()
    nbytes = lib.lqp_boxqp_forward_huber_workspace_bytes(0, 2, 8, 0)
    some_hook = _lib.CHECK_HOOK(lambda user, stream, counters, index: 0)

    def call(w=P, c=P, delta=P, zone=P, u_box=P, ws_bytes=nbytes, hook=None, **ctl_over):
        for k, v in dict(dict(reserved2=0, rho_mode=0, rho_value=0.0), **ctl_over).items():
            setattr(ctl, k, v)
        ctl.check_hook = hook if hook is not None else _lib.CHECK_HOOK()
        return lib.lqp_boxqp_forward_huber(None, 0, 2, 8, 0, P, P, None, None, P, P, w, c, delta, ctypes.byref(ctl), None, P, P, P, P, None, P,
                                           zone, u_box, ctypes.byref(stats), P, ws_bytes)
    for kw in (dict(w=None), dict(c=None), dict(delta=None), dict(zone=None), dict(u_box=None), dict(reserved2=8), dict(reserved2=1),
               dict(hook=some_hook), dict(rho_mode=1, rho_value=0.0), dict(rho_mode=1, rho_value=-1.0)):
        assert call(**kw) == 1, kw
    assert call(ws_bytes=lib.lqp_boxqp_forward_workspace_bytes(0, 2, 8, 0)) == 2
    duals = lambda u_box=P, zone=P, w=P, mode=1, u_e=P, lams_e=P, curv=P: lib.lqp_boxqp_huber_effective_duals(
        None, 0, 2, 8, u_box, zone, w, mode, 1.0, None, u_e, lams_e, curv)
    for kw in (dict(u_box=None), dict(zone=None), dict(w=None), dict(u_e=None), dict(lams_e=None), dict(curv=None), dict(mode=2), dict(mode=3),
               dict(mode=0)):
        assert duals(**kw) == 1, kw
    assert lib.lqp_boxqp_huber_effective_duals(None, 3, 2, 8, P, P, P, 1, 1.0, None, P, P, P) == 1
    for k in range(6):          # (dp, z, zone, w, c, delta)
        a = [P] * 6
        a[k] = None
        assert lib.lqp_boxqp_huber_finish_grads(None, 0, 2, 8, *a, P, P, P) == 1, k
    assert lib.lqp_boxqp_huber_finish_grads(None, 3, 2, 8, P, P, P, P, P, P, P, P, P) == 1
    assert lib.lqp_boxqp_huber_finish_grads(None, 0, 2, 8, P, P, P, P, P, P, None, None, None) == 0          # (no output asked for: nothing to do)
