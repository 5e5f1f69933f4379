"""control['unbounded'] without a GPU: the truth of tests/dinf_table.py, that its rows are decided (both dtypes and the form of Qs x
that does not touch Q agree, every verdict stands clear of the threshold by MARGIN), that the new key cannot change a verdict of the
existing tables, and the rules of the new keys -- the ValueErrors of the Python layer, the new symbols, the argument checks of
lqp_boxqp_forward_certify."""
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
import dinf_table as DT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = list(DT.ROWS)
KEYS = ("x", "z", "u", "lams", "nus", "rho")
NEW = ("lqp_boxqp_forward_certify_workspace_bytes", "lqp_boxqp_forward_certify")
FORMS = {"float32": (torch.float32, False), "float64": (torch.float64, False), "rhs": (torch.float32, True)}


def _same(a, b):
    return (a is None and b is None) or torch.equal(torch.as_tensor(a), torch.as_tensor(b))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ROWS)
def test_every_verdict_is_the_tables_and_stands_clear_of_the_threshold(name, form):
    """status / iters of the table in float32, float64 and (float32) with Qs x formed from the right-hand side; at the detecting check
    the dual rule clears eps by the row's margin (MARGIN; 1.05 on the row that checks at every iteration), at the valid check before it
    misses by it, no problem that is not flagged comes within it at any check; |As dx|_inf / N <= eps at every detecting check -- the test OSQP makes and the kernels leave out"""
    row = DT.ROWS[name]
    t = DT.truth(name, FORMS[form][0], True, FORMS[form][1])
    assert [s["status"] for s in t] == row["status"] and [s["iter"] for s in t] == row["iters"]
    for b, s in enumerate(t):
        clear, miss_before, nearest = DT.margins(s)
        print(name, form, b, "status", s["status"], "iter", s["iter"], "clear", clear, "miss before", miss_before, "nearest", nearest,
              "As dx", s["as_dx"][-1] if s["as_dx"] else None)
        if s["status"] == DT.UNBOUNDED:
            assert clear >= row["margin"], (b, clear)
            assert miss_before is None or miss_before >= row["margin"], (b, miss_before)
            assert s["as_dx"][-1] <= DT.EPS, (b, s["as_dx"][-1])
        assert nearest >= row["margin"], (b, nearest)
        if s["checks"]:                                  # (the mixed row: the primal rule, by infeas_table's measure)
            p_clear, p_before, p_nearest = IT.margins(s)
            assert (p_clear is None or p_clear >= DT.MARGIN) and (p_before is None or p_before >= DT.MARGIN) and p_nearest >= DT.MARGIN
    assert (row["margin"] == DT.MARGIN == 2.0 and row["check"] == 30) or (name == "chunk_n20" and row["margin"] == 1.05 and row["check"] == 1)


@pytest.mark.parametrize("name", ROWS)
def test_what_a_row_is_made_of(name):
    row = DT.ROWS[name]
    B = row["B"]
    assert [b for b in range(B) if row["status"][b] == DT.UNBOUNDED] == sorted(row["gross"] + row["mild"])
    assert [b for b in range(B) if row["status"][b] == DT.INFEASIBLE] == sorted(row["primal"])
    assert row["open"] and all(row["status"][b] == DT.OPTIMAL for b in row["open"])
    assert B <= 8 and row["n"] <= 1030 and row["control"]["max_iters"] <= 1500
    if row["dtype"] == torch.float32:                    # (a drifting iterate keeps every rounding: the x bar is 167 unit roundoffs)
        assert all(row["iters"][b] <= DT.FLAGGED_BY for b in row["gross"] + row["mild"])
    # without the key the unbounded problems run out of iterations (status 1), and their x has grown with the count
    off = DT.truth(name, row["dtype"], False)
    last = row["control"]["max_iters"] - 1
    on = DT.truth(name, row["dtype"])
    for b in row["gross"] + row["mild"]:
        assert off[b]["status"] == DT.MAXITER and off[b]["iter"] == last
        assert float(off[b]["x"].abs().max()) > 2 * float(on[b]["x"].abs().max())
    # the opened box: infinite exactly where the direction points
    Q, p, A, b_, lb, ub = DT.inputs(row)
    for i in row["gross"] + row["mild"] + row["open"]:
        d = DT.direction(row, i, A)
        assert int((d != 0).sum()) == row["m"] + 2
        assert torch.equal(torch.isinf(ub[i, :, 0]), d > 0) and torch.equal(torch.isinf(lb[i, :, 0]), d < 0)
        if A is not None:
            assert float((A[i] @ d).abs().max()) <= 1e-12 * float(d.abs().max()) * float(A[i].abs().max()) * row["n"]
    for i in row["gross"] + row["mild"]:
        d = DT.direction(row, i, A)
        assert float((Q[i] @ d).abs().max()) <= 1e-12 * float(Q[i].abs().max()) * float(d.abs().max()) * row["n"]
        assert float(p[i, :, 0] @ d) < 0


def test_the_event_rows_flag_behind_the_event():
    for name in ("split_n130_event", "big_n1030"):
        row = DT.ROWS[name]
        event = O.resolve_control(DT.control(row), row["n"]).adaptive_rho_iter
        assert event == 30
        for dtype in (torch.float32, torch.float64):
            t = DT.truth(name, dtype)
            for b in row["gross"] + row["mild"]:
                assert t[b]["n_factor"] >= 2 and t[b]["iter"] > event
                assert float(torch.as_tensor(t[b]["rho"]).reshape(-1)[0]) != row["control"]["rho"]
                at = [c for c in t[b]["dchecks"] if c[0] == event]      # the check held with the new rho only refreshes the snapshot
                assert len(at) == 1 and at[0][5] is False


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("table,name", [("infeas", "split_n130"), ("infeas", "f64_n70_m3"), ("dinf", "small_n50"), ("dinf", "mixed_n130")])
def test_with_the_dual_threshold_off_it_is_solve_detect_bit_for_bit(table, name, dtype):
    """with the primal threshold on, and (one row: the flagged problems then run to max_iters) with both off"""
    T = IT if table == "infeas" else DT
    row = T.ROWS[name]
    qp = T.inputs(row, dtype)
    for eps in (IT.EPS, None) if name == "small_n50" else (IT.EPS,):
        for i in range(row["B"]):
            one = E.alone(qp, i)
            ctl = T.control(row, problem=i) if table == "infeas" else T.control(row)
            want = IT.solve_detect(*one, ctl, eps_prim_inf=eps, **E.ALONE)
            got = DT.solve_certify(*one, ctl, eps_prim_inf=eps, eps_dual_inf=None, **E.ALONE)
            assert got["dchecks"] == [] and got["as_dx"] == []
            assert all(got[k] == want[k] for k in ("iter", "status", "checks", "n_factor")), (i, eps)
            assert all(_same(got[k], want[k]) for k in KEYS), (i, eps)


@pytest.mark.parametrize("table,name", [("each", n) for n in E.ROWS] + [("infeas", n) for n in IT.ROWS])
def test_the_new_key_cannot_change_a_verdict_of_the_existing_tables(table, name):
    """every bound of those rows is finite, so max_i(-dx_i, dx_i) = |dx|_inf and e3 = 1 whenever N > 0: the dual rule never holds,
    status and iteration count are the ones without it (the row's own dtype)"""
    T = E if table == "each" else IT
    row = T.ROWS[name]
    qp = T.inputs(row, row["dtype"])
    assert all(bool(torch.isfinite(t).all()) for t in qp[4:])
    prim = IT.EPS if table == "infeas" else None
    for i in range(row["B"]):
        ctl = T.control(row, problem=i) if table == "infeas" else T.control(row)
        got = DT.solve_certify(*E.alone(qp, i), ctl, eps_prim_inf=prim, eps_dual_inf=DT.EPS, **E.ALONE)
        assert all(c[3] > DT.EPS for c in got["dchecks"] if c[4] is not None), (i, got["dchecks"])
        assert got["status"] != DT.UNBOUNDED
        if table == "infeas":
            assert got["status"] == row["status"][i] and got["iter"] == row["iters"][i]
        else:
            assert got["iter"] == row["iters"][i]


# ---- the Python layer ----
def test_resolve_control_and_the_factory():
    r = SB.resolve_control({}, 10)
    assert r["unbounded"] is None and r["eps_dual_inf"] == 1e-4 and r["infeasible"] is None and r["eps_prim_inf"] == 1e-4
    r = SB.resolve_control(dict(stop='each', unbounded='flag', eps_dual_inf=torch.tensor([1e-3])), 10)
    assert r["unbounded"] == 'flag' and r["eps_dual_inf"] == pytest.approx(1e-3) and r["infeasible"] is None
    r = SB.resolve_control(dict(stop='each', unbounded='raise', infeasible='flag'), 10)
    assert (r["unbounded"], r["infeasible"]) == ('raise', 'flag')
    ctl = L.box_qp_control(stop='each', unbounded='raise', eps_dual_inf=1e-5)
    assert ctl["unbounded"] == 'raise' and ctl["eps_dual_inf"] == 1e-5 and "unbounded" not in L.box_qp_control()
    import lqp_py_amd.control as C
    assert "unbounded" in C.__doc__ and "eps_dual_inf" in C.__doc__
    assert "UnboundedQPError" in L.__all__
    err = L.UnboundedQPError("x", [3, 1])
    assert err.indices == [1, 3] and isinstance(err, RuntimeError)
    base = [c for c in L.UnboundedQPError.__mro__ if c in L.InfeasibleQPError.__mro__ and c is not RuntimeError][0]
    assert base is _lib.CertifiedQPError and not issubclass(L.UnboundedQPError, L.InfeasibleQPError)
    assert "says 3" in SB.torch_solve_box_qp.__doc__ and "3 dual infeasible" in SB.torch_solve_box_qp.__doc__
    assert "3" in SB.last_problem_status.__doc__ and "unbounded" in SB.last_problem_status.__doc__


def _refused(ctl, match):
    with pytest.raises(ValueError, match=match):
        L.torch_solve_box_qp(None, None, None, None, None, None, ctl)
    with pytest.raises(ValueError, match=match):
        SB.SolveBoxQPLayer.apply(None, None, None, None, None, None, ctl)
    with pytest.raises(ValueError, match=match):
        SB.check_stop(ctl)


@pytest.mark.parametrize("bad", ['yes', True, 1, 'Flag', ['flag']])
def test_a_bad_mode_is_a_value_error_at_the_call(bad):
    _refused(L.box_qp_control(stop='each', unbounded=bad), "unbounded")


@pytest.mark.parametrize("bad", [0.0, 1.0, -1e-4, 2.0, math.nan, math.inf, "1e-4", None, True, torch.tensor([1e-4, 1e-4])])
def test_a_bad_threshold_is_a_value_error_at_the_call(bad):
    _refused(L.box_qp_control(stop='each', unbounded='flag', eps_dual_inf=bad), "eps_dual_inf")
    _refused(L.box_qp_control(eps_dual_inf=bad), "eps_dual_inf")


def test_the_key_needs_each_and_refuses_unroll():
    for mode in ('raise', 'flag'):
        _refused(L.box_qp_control(unbounded=mode), "stop")
        _refused(L.box_qp_control(unbounded=mode, stop='all'), "stop")
        with pytest.raises(ValueError):
            L.torch_solve_box_qp(None, None, None, None, None, None, L.box_qp_control(unbounded=mode, stop='each', unroll=True))
        with pytest.raises(ValueError, match="unroll"):
            SB.check_infeasible(L.box_qp_control(unbounded=mode, stop='each', unroll=True), 'unbounded', 'eps_dual_inf')
    SB.check_stop(L.box_qp_control(unbounded='flag', stop='each'))
    SB.check_stop(L.box_qp_control(unbounded='flag', infeasible='raise', stop='each'))
    SB.check_stop(L.box_qp_control(unbounded=None))
    SB.check_stop(L.box_qp_control(eps_dual_inf=1e-3))               # (the threshold alone turns nothing on)


# ---- the C ABI ----
def test_header_binding_and_library_agree_on_the_new_symbols():
    text = open(os.path.join(REPO, "include", "lqp_amd.h")).read()
    lib = _lib.load()
    assert lib.lqp_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define LQP_ABI_VERSION (\d+)", text).group(1)) == 17
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        decl = re.search(r"(\w+)\s+%s\s*\((.*?)\)\s*;" % name, flat, flags=re.S)
        assert decl is not None, name
        res, args = _lib.SYMBOLS[name]
        assert len([a for a in decl.group(2).split(",") if a.strip()]) == len(args), name
        assert (decl.group(1) == "size_t") == (res is ctypes.c_size_t)
        assert getattr(lib, name) is not None
    # the certifying call takes the forward's arguments and two trailing doubles
    assert _lib.SYMBOLS["lqp_boxqp_forward_certify"][1][:-2] == _lib.SYMBOLS["lqp_boxqp_forward"][1]
    assert _lib.SYMBOLS["lqp_boxqp_forward_certify"][1][-2:] == [ctypes.c_double, ctypes.c_double]
    assert re.search(r"double\s+eps_prim_inf\s*,\s*double\s+eps_dual_inf\s*\)\s*;", flat)
    # no struct moved: BoxQPCtrl is what it was
    assert _lib.BoxQPCtrl._fields_[-1][0] == "alpha" and ctypes.sizeof(_lib.BoxQPCtrl) == lib.lqp_boxqp_ctrl_bytes()
    assert _lib.RP_INFEAS == 1 << 16 and _lib.RP_UNBOUNDED == 1 << 17 and "bit 17" in text


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("B,n,m", [(1, 4, 0), (8, 130, 1), (6, 130, 17), (2, 1030, 1)])
def test_the_workspace_sizes(dt, B, n, m):
    lib = _lib.load()
    plain, detect = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), lib.lqp_boxqp_forward_detect_workspace_bytes(dt, B, n, m)
    certify = lib.lqp_boxqp_forward_certify_workspace_bytes(dt, B, n, m)
    es = 4 if dt == 0 else 8
    need = B * 2 * (2 * n + m + 4) * es               # detect is what it was (the relation of tests/test_infeas_table.py)
    assert plain + need <= detect <= plain + need + B * 2 * 4 * es + 512
    # ... and the dual certificate's x and Qs x lie in both slots of every problem
    assert detect + B * 2 * 2 * n * es <= certify <= detect + B * 2 * (2 * n + 4) * es + 512
    assert lib.lqp_boxqp_forward_certify_workspace_bytes(7, B, n, m) == 0


def test_forward_certify_refuses_before_it_touches_anything():
    """Dummy pointers that are never dereferenced and a workspace of 0 bytes: a call whose arguments pass ends at the workspace
    check (2), in front of the first use of a device; a bad threshold, both off, a missing bit 3, bit 0 or a hook end before that (1)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)

    def call(eps_p, eps_d, hook=None, **fields):
        ctl = _lib.BoxQPCtrl(max_iters=10, check_solved=1, **fields)
        if hook is not None:
            ctl.check_hook = hook
        return lib.lqp_boxqp_forward_certify(None, 0, 1, 4, 0, fake, fake, None, None, fake, fake, ctypes.byref(ctl), None,
                                             fake, fake, fake, fake, None, fake, None, fake, 0, eps_p, eps_d)
    for ok in ((1e-4, 1e-4), (0.0, 1e-4), (1e-4, 0.0), (0.5, 1e-12)):
        assert call(*ok, reserved2=8) == 2, ok
    assert call(1e-4, 1e-4, reserved2=8 | 4 | 2) == 2
    assert call(0.0, 0.0, reserved2=8) == 1                                  # both off
    for bad in (1.0, -1e-4, math.nan, math.inf, -math.inf, 2.0):
        assert call(bad, 1e-4, reserved2=8) == 1 and call(1e-4, bad, reserved2=8) == 1 and call(0.0, bad, reserved2=8) == 1, bad
    assert call(1e-4, 1e-4) == 1 and call(1e-4, 1e-4, reserved2=4) == 1      # no bit 3
    assert call(1e-4, 1e-4, reserved2=8 | 1) == 1                            # bit 0: the factor kept for the unroll sweep
    hook = _lib.CHECK_HOOK(lambda *_a: 0)
    assert call(1e-4, 1e-4, hook=hook, reserved2=8) == 1
    # the detecting entry point is what it was
    ctl = _lib.BoxQPCtrl(max_iters=10, check_solved=1, reserved2=8)
    assert lib.lqp_boxqp_forward_detect(None, 0, 1, 4, 0, fake, fake, None, None, fake, fake, ctypes.byref(ctl), None,
                                        fake, fake, fake, fake, None, fake, None, fake, 0, 1e-4) == 2
