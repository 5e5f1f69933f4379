"""CPU checks of tests/kkt_table.py and of the oracle's KKT-system backward (oracle.boxqp_oracle.solve_box_qp_grad_kkt), which
together pin backward='kkt': the oracle reproduces the reference-made golden g12, its reduced system is its full (3n+m) system,
its bookkeeping of one-sided batches is the reference's, the rows cover every block-count threshold and every backward knob the
KKT path reads, and the comparator of tests/test_gpu_kkt.py sees a one-tile error of Q, swapped multipliers and a missing clamp."""
import math

import pytest
import torch

import kkt_table as KT
import tier_table as T
from conftest import load_golden
from oracle import boxqp_oracle as O
from test_tier_table import documented_knobs

CUS = 256          # (any count: the GPU module reads the real one)
TOL = dict(eps_abs=1e-5, eps_rel=1e-5)


def _scale(t):
    return max(1.0, float(t.abs().max()))


def _sampled_point(r):
    B = T.batch(r, CUS)
    return KT.point(r, B, T.sample(B))


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle
def test_oracle_reproduces_the_golden_kkt_backward():
    """The oracle's own float32 forward at the golden's tolerances, then its KKT backward: the reference's gradients within the
    1e-4 of scale test_g12_kkt_backward_mode asks of the GPU (measured: 2e-6 of scale at most, x bit for bit), with and without the
    equality rows."""
    g = load_golden("g12_kkt_backward")
    n = g["Q"].shape[1]
    for tag, A, b in (("", g["A"], g["b"]), ("_box", None, None)):
        sol = O.solve_box_qp(g["Q"], g["p"], A, b, g["lb"], g["ub"], O.make_control(**TOL))
        assert float((sol["x"] - g["x" + tag]).abs().max()) < 2e-5
        got = dict(zip(KT.GRADS, O.solve_box_qp_grad_kkt(g["cot"], sol["x"], sol["lams"], sol["nus"], g["Q"], A, g["lb"], g["ub"])))
        for k in KT.GRADS:
            if A is None and k in ("dA", "db"):
                assert got[k] is None
                continue
            want = g[k + tag]
            e = float((got[k] - want).abs().max()) / _scale(want)
            print(f"g12{tag} {k}: {e:.3e} of scale")
            assert got[k].shape == want.shape and e < 1e-4, (tag, k, e)
        assert n == 40


FULL_ROWS = [r["name"] for r in KT.ROWS if r["n"] <= 257]


@pytest.mark.parametrize("name", FULL_ROWS)
def test_full_system_is_the_reduced_system(name):
    """float64: the reference's literal (3n+m) system (rows of infinite slack dropped) against its (n+m) reduction on the row's
    point, within 1e-10 of scale -- three orders above the 1.4e-13 measured on these rows, three below the float32 budget it protects.  The truth
    is finite (no entry is masked anywhere)."""
    r = KT.ROW_BY_NAME[name]
    pt = _sampled_point(r)
    red = KT.oracle(pt, torch.float64, "reduced")
    full = KT.oracle(pt, torch.float64, "full")
    for k in KT.GRADS:
        assert (red[k] is None) == (full[k] is None) == KT.none_pattern(r)[k], k
        if red[k] is not None:
            assert torch.isfinite(red[k]).all(), k
            e = float((red[k] - full[k]).abs().max()) / _scale(red[k])
            assert e <= 1e-10, (k, e)


@pytest.mark.parametrize("name", [r["name"] for r in KT.ROWS])
def test_truth_is_finite_and_points_are_what_the_table_says(name):
    r = KT.ROW_BY_NAME[name]
    pt = _sampled_point(r)
    cot, x, lams, nus, Q, A, lb, ub = pt
    n = r["n"]
    assert (bool(torch.isfinite(lb).any()), bool(torch.isfinite(ub).any())) == KT.flags(r)
    assert bool((x >= lb).all()) and bool((x <= ub).all()) and bool((lams >= 0).all())
    assert bool((lams[:, :n] * lams[:, n:] == 0).all())
    t64 = KT.oracle(pt, torch.float64)
    for k in KT.GRADS:
        assert (t64[k] is None) == KT.none_pattern(r)[k], k
        assert t64[k] is None or bool(torch.isfinite(t64[k]).all()), k
    if n >= 63 and r["sides"] == "both":
        # every kind of variable the table promises: at a bound with a multiplier, both clamps acting, fixed, 1e-6 inside
        s_lo, s_hi = x - lb, ub - x
        assert bool(((s_lo == 0) & (lams[:, :n] > 0)).any()) and bool(((s_hi == 0) & (lams[:, n:] > 0)).any())
        assert bool(((s_hi == 0) & (lams[:, n:] == 0) & (s_lo > 0)).any())
        assert bool(((s_lo == 0) & (s_hi == 0)).any())
        assert bool(((s_lo > 0) & (s_lo < 2e-6)).any())
        w = torch.clamp(lams[:, :n], min=1e-8) / torch.clamp(s_lo, min=1e-8) + torch.clamp(lams[:, n:], min=1e-8) / torch.clamp(s_hi, min=1e-8)
        assert float(w.min()) < 1e-7 and float(w.max()) > 1e6
    if r["q"] == "sym":
        assert torch.equal(Q, Q.transpose(1, 2))


def test_indefinite_row_fails_cholesky_and_solves():
    """The fallback row: Q + diag(w) is not positive definite in float32 (torch.linalg.cholesky refuses), the KKT system is far
    from singular (float64 solve, condition number of the equilibrated system)."""
    r = KT.ROW_BY_NAME["fallback_indef_n200"]
    cot, x, lams, nus, Q, A, lb, ub = KT.point(r, T.batch(r, CUS))
    n = r["n"]
    assert torch.equal(Q, Q.transpose(1, 2))
    w = (torch.clamp(lams[:, :n], min=1e-8) / torch.clamp(x - lb, min=1e-8) + torch.clamp(lams[:, n:], min=1e-8) / torch.clamp(ub - x, min=1e-8))
    Qw = Q + torch.diag_embed(w.squeeze(2))
    _, info = torch.linalg.cholesky_ex(Qw)
    assert bool((info > 0).all()), info
    assert float(torch.linalg.eigvalsh(Qw.double()).min()) < -0.4
    K = O.kkt_matrix(Qw.double(), A.double())
    d = K.diagonal(dim1=1, dim2=2).abs().clamp(min=1.0).rsqrt()
    cond = torch.linalg.cond(d.unsqueeze(2) * K * d.unsqueeze(1))
    assert float(cond.max()) < 1e5, cond
    t64 = KT.oracle((cot, x, lams, nus, Q, A, lb, ub), torch.float64)
    assert all(bool(torch.isfinite(t64[k]).all()) for k in KT.GRADS)


def test_sides_bookkeeping_by_hand():
    """Three variables, Q = I, no equality rows: dx_i = -g_i / (1 + w_i), dlam_lo = -dx / s_lo, dlam_hi = dx / s_hi, written out."""
    Q = torch.eye(3, dtype=torch.float64).unsqueeze(0)
    g = torch.tensor([[[1.0], [2.0], [-3.0]]], dtype=torch.float64)
    x = torch.tensor([[[0.5], [-1.0], [2.0]]], dtype=torch.float64)
    lb = torch.tensor([[[0.0], [-1.0], [-4.0]]], dtype=torch.float64)
    ub = torch.tensor([[[1.0], [3.0], [2.0]]], dtype=torch.float64)
    lams = torch.tensor([[[0.0], [0.5], [0.0], [0.0], [0.0], [0.25]]], dtype=torch.float64)
    inf = torch.full_like(lb, math.inf)
    c = 1e-8
    for sides in KT.SIDES:
        l = lb if sides in ("both", "lb") else -inf
        u = ub if sides in ("both", "ub") else inf
        dQ, dp, dA, db, dlb, dub, last = O.solve_box_qp_grad_kkt(g, x, lams, None, Q, None, l, u)
        assert dA is None and db is None and last is None
        if sides == "none":
            w = [0.0, 0.0, 0.0]                       # no G at all: the clamped multipliers do not enter
        else:
            s_lo = [0.5, c, 6.0] if sides != "ub" else [math.inf] * 3
            s_hi = [0.5, 4.0, c] if sides != "lb" else [math.inf] * 3
            l_lo, l_hi = [c, 0.5, c], [c, c, 0.25]
            w = [l_lo[i] / s_lo[i] + l_hi[i] / s_hi[i] for i in range(3)]
        dx = [-float(g[0, i, 0]) / (1.0 + w[i]) for i in range(3)]
        assert torch.allclose(dp[0, :, 0], torch.tensor(dx, dtype=torch.float64), rtol=1e-13, atol=0)
        xs = [0.5, -1.0, 2.0]
        for i in range(3):
            for j in range(3):
                assert math.isclose(float(dQ[0, i, j]), 0.5 * (dx[i] * xs[j] + xs[i] * dx[j]), rel_tol=1e-13, abs_tol=1e-300)
        if sides == "none":
            assert dlb is None and dub is None
            continue
        # dl_dh = -lam * dlam: lower half -l_lo * (-dx / s_lo), upper half -l_hi * (dx / s_hi)
        h_lo = [l_lo[i] * dx[i] / s_lo[i] for i in range(3)]
        h_hi = [-l_hi[i] * dx[i] / s_hi[i] for i in range(3)]
        if sides == "both":
            want_lb, want_ub = [-v for v in h_lo], h_hi
        elif sides == "lb":
            want_lb, want_ub = [-v for v in h_lo], None
        else:
            want_lb, want_ub = None, h_lo              # the reference's quirk: the LOWER half, all zeros (s_lo = inf)
            assert all(v == 0.0 for v in h_lo)
        for got, want in ((dlb, want_lb), (dub, want_ub)):
            assert (got is None) == (want is None), sides
            if want is not None:
                assert torch.allclose(got[0, :, 0], torch.tensor(want, dtype=torch.float64), rtol=1e-13, atol=0), (sides, got, want)
        if sides == "both":                            # ... and the full system agrees on the hand-made example too
            full = O.solve_box_qp_grad_kkt(g, x, lams, None, Q, None, l, u, form="full")
            for a, b in zip((dQ, dp, dlb, dub), (full[0], full[1], full[4], full[5])):
                assert float((a - b).abs().max()) <= 1e-10 * _scale(a)


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
def backward_knobs():
    return sorted(k for k in documented_knobs() if k.startswith("LQP_BWD_") or k in KT.BACKWARD_KNOBS_EXTRA)


def uncovered_knobs(rows):
    knobs = documented_knobs()
    forced = {k for r in rows for k, v in r["env"].items() if v != knobs.get(k)}
    return sorted(k for k in backward_knobs() if k not in KT.NOT_READ and k not in forced)


def uncovered_thresholds(rows):
    missing = []
    for what, (key, lo, hi) in KT.THRESHOLDS.items():
        vals = {KT.threshold_value(key, r) for r in rows}
        if not (lo in vals and hi in vals):
            missing.append(what)
    return missing


def test_rows_cover_every_backward_knob_and_threshold():
    knobs = documented_knobs()
    assert len(backward_knobs()) >= 10, backward_knobs()
    assert set(KT.NOT_READ) <= set(backward_knobs()) and all(KT.NOT_READ.values())
    for r in KT.ROWS:
        assert set(r["env"]) <= set(knobs) and set(r["flip"] or {}) <= set(knobs), r["name"]
        assert r["dtype"] in ("f32", "f64") and r["entry"] in KT.ENTRIES and r["sides"] in KT.SIDES and r["form"] in KT.FORMS, r["name"]
        assert r["q"] in ("sym", "nonsym", "indef") and T.batch(r, CUS) >= 1, r["name"]
        assert r["R"] <= T.R_MAX and r["F"] <= T.F_MAX, r["name"]
        if (r["R"], r["F"]) != (T.R_DEFAULT, T.F_DEFAULT) or r["same"]:
            assert r["why"] and "measured" in r["why"], (r["name"], "a raised bar or a same-bits flip needs its measured reason")
        if r["dtype"] == "f64" or r["q"] == "nonsym":
            assert r["form"] in ("lu", "composed"), r["name"]       # (the Cholesky form is float32 on a symmetric Q)
        if r["form"] == "chol":
            assert r["entry"] == "chol" and r["n"] <= 1024 and r["m"] <= 16, r["name"]
        assert (r["form"] == "composed") == (r["entry"] == "composed"), r["name"]
        if r["n"] >= 1000 and isinstance(r["B"], int):
            assert r["B"] <= 2, r["name"]                           # (the oracle's cost)
    assert uncovered_knobs(KT.ROWS) == []
    assert uncovered_thresholds(KT.ROWS) == []
    # every kind of batch on both native entries, the symbolic batch size, both composed dtypes, one `want` row
    for entry in ("chol", "lu"):
        assert {r["sides"] for r in KT.ROWS if r["entry"] == entry} == set(KT.SIDES), entry
    assert "cus + 3" in {r["B"] for r in KT.ROWS} and 1 in {r["B"] for r in KT.ROWS}
    assert {r["dtype"] for r in KT.ROWS if r["entry"] == "composed"} == {"f32", "f64"}
    assert any(r["want"] and r["entry"] == "chol" and r["sides"] == "both" and r["m"] > 0 for r in KT.ROWS)
    assert [r["name"] for r in KT.ROWS if r["form"] == "fallback"] == ["fallback_indef_n200"]


def test_coverage_check_fails_without_its_rows():
    """The coverage check is not vacuous: without the only row that forces a knob, or without one side of a threshold, it fails."""
    knob_rows = {}
    for r in KT.ROWS:
        for k in r["env"]:
            knob_rows.setdefault(k, []).append(r["name"])
    singles = [k for k, v in sorted(knob_rows.items()) if len(v) == 1]
    assert singles
    for only in singles:
        assert uncovered_knobs([r for r in KT.ROWS if r["name"] != knob_rows[only][0]]) == [only]
    for what, (key, lo, hi) in KT.THRESHOLDS.items():
        for side in (lo, hi):
            assert what in uncovered_thresholds([r for r in KT.ROWS if KT.threshold_value(key, r) != side]), (what, side)


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator
SENS_ROWS = [r["name"] for r in KT.ROWS if r["dtype"] == "f32" and 64 <= r["n"] <= 513]


def _swap_halves(args):
    n = args[1].shape[1]
    args = list(args)
    args[2] = torch.cat((args[2][:, n:], args[2][:, :n]), 1)
    return args


def _perturb_q(args):
    args = list(args)
    args[4] = T.perturb_last_block(args[4])
    return args


@pytest.mark.parametrize("name", SENS_ROWS)
def test_comparator_sees_errors(name):
    """With the oracle's float32 backward standing in for the GPU's the row passes at its own R and F; it fails with the last
    diagonal 64-block of Q scaled by 1 + 1e-4, with the lower and upper halves of lams swapped, and with the clamp of the slacks
    left out."""
    from functools import partial
    r = KT.ROW_BY_NAME[name]
    pt = _sampled_point(r)
    t64 = KT.oracle(pt, torch.float64)
    t32 = KT.oracle(pt, torch.float32)
    ok = KT.compare(r, t32, t32, t64)
    assert all(rec["ok"] for rec in ok.values()) and {"dQ", "dp"} <= set(ok), ok
    args32 = [None if t is None else t.float() for t in pt]
    wrong = {
        "one tile of Q": KT.oracle(pt, torch.float32, hook=_perturb_q),
        "lams halves swapped": KT.oracle(pt, torch.float32, hook=_swap_halves),
        "no clamp of the slacks": dict(zip(KT.GRADS, O.solve_box_qp_grad_kkt(*args32, slack_floor=0.0)[:6])),
    }
    for what, w in wrong.items():
        if what != "one tile of Q" and r["sides"] == "none":
            continue                                   # (no finite bound: neither multipliers nor slacks enter, :453)
        res = KT.compare(r, w, t32, t64)
        assert not all(rec["ok"] for rec in res.values()), (what, {k: (v["err"], v["bar"]) for k, v in res.items()})
