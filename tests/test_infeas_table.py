"""control['infeasible'] without a GPU: the truth of tests/infeas_table.py, that its rows are decided (both dtypes agree, every
verdict stands clear of the threshold by the row's factor), and the rules of the new keys -- the ValueErrors of the Python layer,
the new symbols, the argument checks of lqp_boxqp_forward_detect."""
import ctypes
import math
import os
import re

import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import each_table as E
import infeas_table as IT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("x", "z", "u", "lams", "nus", "rho")
ROWS = list(IT.ROWS)
NEW = ("lqp_boxqp_forward_detect_workspace_bytes", "lqp_boxqp_forward_detect", "lqp_boxqp_problem_status")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["small_n50", "split_n130_event", "f64_n70_m3"])
def test_the_restatement_without_detection_is_the_oracle(name, dtype):
    """every problem of a row (the infeasible ones run out of iterations), bit for bit: solve_detect attaches its callback with both
    thresholds off, the oracle here runs without one"""
    row = IT.ROWS[name]
    qp = IT.inputs(row, dtype)
    off = IT.truth(name, dtype, False)
    for i in range(row["B"]):
        trace = {}
        want = O.solve_box_qp(*E.alone(qp, i), IT.control(row, problem=i), trace=trace, **E.ALONE)
        got = off[i]
        assert got["iter"] == want["iter"] and got["checks"] == [] and got["n_factor"] == trace["n_factor"]
        assert got["status"] == trace["status"] == (IT.OPTIMAL if want["iter"] < row["control"]["max_iters"] - 1 else IT.MAXITER)
        for k in KEYS:
            a, b = got[k], want[k]
            assert (a is None and b is None) or torch.equal(torch.as_tensor(a), torch.as_tensor(b)), (i, k)


def test_the_oracle_refuses_a_per_check_callback_next_to_a_check_hook():
    qp = E.inputs(E.ROWS["chunk_n20"], torch.float64)
    with pytest.raises(ValueError, match="at_check"):
        O.solve_box_qp(*qp, E.control(E.ROWS["chunk_n20"]), check_hook=lambda counts, k: None, at_check=lambda it, state: 0)


def test_a_callback_that_never_flags_changes_no_bit():
    """through an adaptive-rho event, in both dtypes; it is called at every check that was not optimal, and at no other"""
    name = "split_n130_event"
    row = E.ROWS[name]
    check = O.resolve_control(E.control(row), row["n"]).check_solved
    for dtype in (torch.float32, torch.float64):
        qp = E.inputs(row, dtype)
        plain = E.solo(name, dtype)
        assert [s["n_factor"] > 1 for s in plain] == row["adapts"] and any(row["adapts"])
        for i in range(row["B"]):
            seen, trace = [], {}
            got = O.solve_box_qp(*E.alone(qp, i), E.control(row), trace=trace, at_check=lambda it, state: seen.append(it) or 0, **E.ALONE)
            assert got["iter"] == plain[i]["iter"] == row["iters"][i] and trace["n_factor"] == plain[i]["n_factor"]
            assert trace["status"] == 0 and seen == list(range(0, got["iter"], check)), (i, seen)      # (the last check is the optimal one)
            for k in KEYS:
                assert (got[k] is None and plain[i][k] is None) or torch.equal(torch.as_tensor(got[k]), torch.as_tensor(plain[i][k])), (i, k)


def test_the_trace_says_how_a_solve_ended():
    """0: it stopped by itself; 1: it ran to max_iters - 1 -- the row that has both"""
    row = E.ROWS["chunk_n20"]
    qp = E.inputs(row, row["dtype"])
    last = row["control"]["max_iters"] - 1
    status = []
    for i in range(row["B"]):
        trace = {}
        sol = O.solve_box_qp(*E.alone(qp, i), E.control(row), trace=trace, **E.ALONE)
        assert sol["iter"] == row["iters"][i] and "status" not in sol
        status.append(trace["status"])
    assert status == [1 if it == last else 0 for it in row["iters"]] and set(status) == {0, 1}


@pytest.mark.parametrize("name", ROWS)
def test_float32_and_float64_truth_agree_on_every_verdict(name):
    row = IT.ROWS[name]
    for dtype in (torch.float32, torch.float64):
        t = IT.truth(name, dtype)
        assert [s["status"] for s in t] == row["status"], dtype
        assert [s["iter"] for s in t] == row["iters"], dtype
    # what the row is made of: the chosen problems are flagged and nobody else is; without the key they run out of iterations
    bad = sorted(row["gross"] + row["mild"])
    assert [b for b in range(row["B"]) if row["status"][b] == IT.INFEASIBLE] == bad
    off = IT.truth(name, row["dtype"], False)
    assert all(off[b]["status"] == IT.MAXITER and off[b]["iter"] == row["control"]["max_iters"] - 1 for b in bad)
    assert row["B"] <= 8 and row["control"]["max_iters"] <= 1500


@pytest.mark.parametrize("form", ["product", "rhs"])
@pytest.mark.parametrize("name", ROWS)
def test_every_verdict_stands_clear_of_the_threshold(name, form):
    """At the detecting check c1 and -c2 clear eps_prim_inf by the row's factor, at the valid check before the rule misses by it, and
    no check of a feasible problem comes within it -- in both dtypes, and (float32, `rhs`) with the certificate's Qs x formed as
    w - rho x - As^T nu, the form of a kernel that does not touch Q, with the same verdicts at the same checks."""
    row = IT.ROWS[name]
    if form == "rhs":
        qp = IT.inputs(row, torch.float32)
        sols = [[IT.solve_detect(*E.alone(qp, i), IT.control(row, problem=i), eps_prim_inf=IT.EPS, qx_from_rhs=True, **E.ALONE)
                 for i in range(row["B"])]]
    else:
        sols = [IT.truth(name, torch.float32), IT.truth(name, torch.float64)]
    for t in sols:
        assert [s["status"] for s in t] == row["status"] and [s["iter"] for s in t] == row["iters"]
        for b, s in enumerate(t):
            clear, miss_before, nearest = IT.margins(s)
            print(name, form, b, "status", s["status"], "iter", s["iter"], "clear", clear, "miss before", miss_before, "nearest", nearest)
            if s["status"] == IT.INFEASIBLE:
                assert clear >= row["margin"], (b, clear)
                assert miss_before is None or miss_before >= row["margin"], (b, miss_before)
            assert nearest >= row["margin"], (b, nearest)
    assert row["margin"] == IT.MARGIN or name == "chunk_n20"


def test_the_event_rows_flag_behind_the_event():
    for name in ("split_n130_event", "big_n1030"):
        row = IT.ROWS[name]
        event = O.resolve_control(IT.control(row), row["n"]).adaptive_rho_iter       # (100; 90 where a check is held every 30)
        for dtype in (torch.float32, torch.float64):
            t = IT.truth(name, dtype)
            for b in row["gross"] + row["mild"]:
                assert t[b]["n_factor"] == 2 and t[b]["iter"] > event
                # the check held with the new rho only refreshes the snapshot
                at = [c for c in t[b]["checks"] if c[0] == event]
                assert len(at) == 1 and at[0][4] is False


# ---- the Python layer ----
def test_resolve_control_and_the_factory():
    assert SB.resolve_control({}, 10)["infeasible"] is None and SB.resolve_control({}, 10)["eps_prim_inf"] == 1e-4
    r = SB.resolve_control(dict(stop='each', infeasible='flag', eps_prim_inf=torch.tensor([1e-3])), 10)
    assert r["infeasible"] == 'flag' and r["eps_prim_inf"] == pytest.approx(1e-3)
    assert SB.resolve_control(dict(infeasible=None), 10)["infeasible"] is None
    ctl = L.box_qp_control(stop='each', infeasible='raise', eps_prim_inf=1e-5)
    assert ctl["infeasible"] == 'raise' and ctl["eps_prim_inf"] == 1e-5 and "infeasible" not in L.box_qp_control()
    import lqp_py_amd.control as C
    assert "infeasible" in C.__doc__ and "eps_prim_inf" in C.__doc__          # (box_qp_control documents the keys)
    assert issubclass(L.InfeasibleQPError, RuntimeError) and L.InfeasibleQPError("x", [3, 1]).indices == [1, 3]


def _refused(ctl, match):
    with pytest.raises(ValueError, match=match):
        L.torch_solve_box_qp(None, None, None, None, None, None, ctl)
    with pytest.raises(ValueError, match=match):
        SB.SolveBoxQPLayer.apply(None, None, None, None, None, None, ctl)
    with pytest.raises(ValueError, match=match):
        SB.check_stop(ctl)


@pytest.mark.parametrize("bad", ['yes', True, 1, 'Flag', ['flag']])
def test_a_bad_mode_is_a_value_error_at_the_call(bad):
    _refused(L.box_qp_control(stop='each', infeasible=bad), "infeasible")


@pytest.mark.parametrize("bad", [0.0, 1.0, -1e-4, 2.0, math.nan, math.inf, "1e-4", None, True, torch.tensor([1e-4, 1e-4])])
def test_a_bad_threshold_is_a_value_error_at_the_call(bad):
    _refused(L.box_qp_control(stop='each', infeasible='flag', eps_prim_inf=bad), "eps_prim_inf")
    _refused(L.box_qp_control(eps_prim_inf=bad), "eps_prim_inf")


def test_the_key_needs_each_and_refuses_unroll():
    for mode in ('raise', 'flag'):
        _refused(L.box_qp_control(infeasible=mode), "stop")
        _refused(L.box_qp_control(infeasible=mode, stop='all'), "stop")
        with pytest.raises(ValueError):
            L.torch_solve_box_qp(None, None, None, None, None, None, L.box_qp_control(infeasible=mode, stop='each', unroll=True))
        with pytest.raises(ValueError, match="unroll"):
            SB.check_infeasible(L.box_qp_control(infeasible=mode, stop='each', unroll=True))
    SB.check_stop(L.box_qp_control(infeasible='flag', stop='each'))
    SB.check_stop(L.box_qp_control(infeasible=None))
    SB.check_stop(L.box_qp_control(eps_prim_inf=1e-3))             # (the threshold alone turns nothing on)


# ---- the C ABI ----
def test_header_binding_and_library_agree_on_the_new_symbols():
    text = open(os.path.join(REPO, "include", "lqp_amd.h")).read()
    lib = _lib.load()
    assert lib.lqp_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define LQP_ABI_VERSION (\d+)", text).group(1)) == 17
    assert "added within ABI 17" in text
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        decl = re.search(r"(\w+)\s+%s\s*\((.*?)\)\s*;" % name, flat, flags=re.S)
        assert decl is not None, name
        res, args = _lib.SYMBOLS[name]
        assert len([a for a in decl.group(2).split(",") if a.strip()]) == len(args), name
        assert (decl.group(1) == "size_t") == (res is ctypes.c_size_t)
        assert getattr(lib, name) is not None
    # the detecting call takes the forward's arguments and one trailing double
    assert _lib.SYMBOLS["lqp_boxqp_forward_detect"][1][:-1] == _lib.SYMBOLS["lqp_boxqp_forward"][1]
    assert _lib.SYMBOLS["lqp_boxqp_forward_detect"][1][-1] is ctypes.c_double
    assert re.search(r"double\s+eps_prim_inf\s*\)\s*;", flat)
    assert _lib.BoxQPCtrl._fields_[-1][0] == "alpha" and ctypes.sizeof(_lib.BoxQPCtrl) == lib.lqp_boxqp_ctrl_bytes()
    assert _lib.RP_INFEAS == 1 << 16


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("B,n,m", [(1, 4, 0), (8, 130, 1), (6, 130, 17), (2, 1030, 1)])
def test_the_snapshots_lie_behind_the_forward_layout(dt, B, n, m):
    lib = _lib.load()
    plain, detect = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), lib.lqp_boxqp_forward_detect_workspace_bytes(dt, B, n, m)
    es = 4 if dt == 0 else 8
    need = B * 2 * (2 * n + m + 4) * es               # two slots of (y, g, nu) and four words per problem
    assert plain + need <= detect <= plain + need + B * 2 * 4 * es + 512
    assert lib.lqp_boxqp_forward_detect_workspace_bytes(7, B, n, m) == 0


def test_forward_detect_refuses_before_it_touches_anything():
    """Dummy pointers that are never dereferenced and a workspace of 0 bytes: a call whose arguments pass ends at the workspace
    check (2), in front of the first use of a device; a bad threshold, a missing bit 3, bit 0 or a hook end before that (1)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)

    def call(eps, hook=None, **fields):
        ctl = _lib.BoxQPCtrl(max_iters=10, check_solved=1, **fields)
        if hook is not None:
            ctl.check_hook = hook
        return lib.lqp_boxqp_forward_detect(None, 0, 1, 4, 0, fake, fake, None, None, fake, fake, ctypes.byref(ctl), None,
                                            fake, fake, fake, fake, None, fake, None, fake, 0, eps)
    assert call(1e-4, reserved2=8) == 2 and call(0.5, reserved2=8 | 4 | 2) == 2 and call(1e-12, reserved2=8) == 2
    for bad in (0.0, 1.0, -1e-4, math.nan, math.inf, -math.inf, 2.0):
        assert call(bad, reserved2=8) == 1, bad
    assert call(1e-4) == 1 and call(1e-4, reserved2=4) == 1                 # no bit 3
    assert call(1e-4, reserved2=8 | 1) == 1                                # bit 0: the factor kept for the unroll sweep
    hook = _lib.CHECK_HOOK(lambda *_a: 0)
    assert call(1e-4, hook=hook, reserved2=8) == 1
    # the plain entry point is what it was
    ctl = _lib.BoxQPCtrl(max_iters=10, check_solved=1, reserved2=8)
    assert lib.lqp_boxqp_forward(None, 0, 1, 4, 0, fake, fake, None, None, fake, fake, ctypes.byref(ctl), None,
                                 fake, fake, fake, fake, None, fake, None, fake, 0) == 2


def test_problem_status_refuses_an_unknown_workspace():
    lib = _lib.load()
    out = (ctypes.c_int32 * 4)()
    assert lib.lqp_boxqp_problem_status(None, 0, 4, 8, 0, ctypes.c_void_p(8192), 1 << 20, out) == 1     # (no forward with bit 3 ran on it)
    assert lib.lqp_boxqp_problem_status(None, 0, 4, 8, 0, None, 1 << 20, out) == 1
    assert lib.lqp_boxqp_problem_status(None, 0, 4, 8, 0, ctypes.c_void_p(8192), 1 << 20, None) == 1
