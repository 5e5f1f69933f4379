"""CPU checks of tests/fp_table.py and of the oracle's fixed-point backward (oracle.boxqp_oracle.solve_box_qp_grad), which together
pin lqp_boxqp_backward_fp: every row's free set has the size the row asks for, in float32 as in float64; the float32 budget is not
zero where the truth is not; the oracle's full (n + m) system is a hand-written reduced solve on the free set; a three-variable
case written out by hand; the rows cover every block-count threshold, entry point, kind of rho and backward knob; and the
comparator of tests/test_gpu_fp.py sees a tie moved into the active set, a wrong sign of dlb / dub, an ignored rho, a one-tile
error of Q and a negated u."""
import pytest
import torch

import fp_table as FT
import tier_table as T
from oracle import boxqp_oracle as O
from test_tier_table import documented_knobs

CUS = 256          # (any count: the GPU module reads the real one)
NAMES = [r["name"] for r in FT.ROWS]


def _scale(t):
    return max(1.0, float(t.abs().max()))


_points = {}


def _sampled(r):
    """(sampled problem indices, their point), built once per row and left unchanged."""
    if r["name"] not in _points:
        B = T.batch(r, CUS)
        idx = T.sample(B)
        _points[r["name"]] = (idx, FT.point(r, B, idx))
    return _points[r["name"]]


# ---------------------------------------------------------------------------------------------------------------------------------
# the points
@pytest.mark.parametrize("name", NAMES)
def test_free_set_has_the_size_the_row_asks_for(name):
    """A condition, not a measurement: exactly nf free variables per problem, the same set in float32 and float64 (float32 rows:
    the budget and the GPU see float32), the last variable free whenever nf > 0, multipliers only on active variables."""
    r = FT.ROW_BY_NAME[name]
    idx, pt = _sampled(r)
    cot, x, u, lams, nus, Q, A, lb, ub, rho = pt
    n = r["n"]
    f64 = FT.free_set(pt, torch.float64)
    assert f64.sum(1).tolist() == [FT.nf_of(r, i) for i in idx]
    if r["dtype"] == "f32":
        assert torch.equal(FT.free_set(pt, torch.float32), f64)
    for k, i in enumerate(idx):
        assert bool(f64[k, n - 1]) == (FT.nf_of(r, i) > 0)
    free = f64.unsqueeze(2)
    assert bool((x >= lb).all()) and bool((x <= ub).all()) and bool((lams >= 0).all())
    assert bool((u[free] == 0).all()) and bool((lams[:, :n][free] == 0).all()) and bool((lams[:, n:][free] == 0).all())
    act = ~free
    assert bool(((lams[:, :n] > 0) ^ (lams[:, n:] > 0))[act].all()) and bool((u[act] != 0).all())
    assert bool(((u * 64) == (u * 64).round()).all()) and float(u.abs().max()) <= 1.0
    fixed = (lb == ub)
    if all(FT.nf_of(r, i) <= n - int(fixed[k].sum()) for k, i in enumerate(idx)):
        assert bool(act[fixed].all())                  # (lb == ub variables are active wherever nf leaves room)
    if any(3 < FT.nf_of(r, i) for i in idx):
        assert bool((free & ((x == ub) | (x == lb))).any())      # free variables exactly on a finite bound
    if n >= 64:
        assert bool(torch.isinf(lb).any()) and bool(torch.isinf(ub).any())
    if r["q"] != "nonsym":
        assert torch.equal(Q, Q.transpose(1, 2))
    if r["rho"] == "tensor" and len(idx) > 1:
        assert rho.shape == (len(idx), 1, 1) and len(set(rho.flatten().tolist())) > 1


@pytest.mark.parametrize("name", NAMES)
def test_float32_budget_is_not_zero_where_the_truth_is_not(name):
    """|t32 - t64| > 0 for every gradient whose truth is not zero: the bar R |t32 - t64| + F scale is the budget's, not F's alone.
    The rows of ZERO_BUDGET are the exception for dQ, dp, dA, db: every free set empty, dv = 0 and dnu = 0 exactly in both."""
    r = FT.ROW_BY_NAME[name]
    idx, pt = _sampled(r)
    t64 = FT.oracle(pt, torch.float64)
    assert (name in FT.ZERO_BUDGET) == (FT.nf_values(r) == {0})
    for k in FT.GRADS:
        assert (t64[k] is None) == FT.none_pattern(r)[k], k
        assert t64[k] is None or bool(torch.isfinite(t64[k]).all()), k
    if name in FT.ZERO_BUDGET:
        for k in ("dQ", "dp", "dA", "db"):
            assert t64[k] is None or not bool(t64[k].any()), k
    if r["dtype"] != "f32":
        return
    t32 = FT.oracle(pt, torch.float32)
    for k in FT.GRADS:
        if t64[k] is None:
            continue
        e32 = float((t32[k].double() - t64[k]).abs().max())
        if name in FT.ZERO_BUDGET and k in ("dQ", "dp", "dA", "db"):
            assert e32 == 0.0, k
        elif bool(t64[k].any()):
            assert e32 > 0.0, k
        assert e32 <= 1e-4 * _scale(t64[k]), (k, e32)        # ... and the point is well conditioned: a usable yardstick


def test_indefinite_row_fails_cholesky_and_solves():
    """The fallback row: Q_FF is not positive definite in float32 (torch.linalg.cholesky refuses), the truth is finite."""
    r = FT.ROW_BY_NAME["fallback_indef_n200"]
    idx, pt = _sampled(r)
    free = FT.free_set(pt, torch.float32)
    for k in range(len(idx)):
        F = free[k].nonzero().squeeze(1)
        Qff = pt[5][k][F][:, F]
        assert int(torch.linalg.cholesky_ex(Qff)[1]) > 0
        assert float(torch.linalg.eigvalsh(Qff.double()).min()) < -0.4
    assert [r["name"] for r in FT.ROWS if r["form"] == "fallback"] == ["fallback_indef_n200"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle
def _reduced(pt):
    """The fixed-point backward written out on the free set, float64: Kf = Q_FF + eps I, u0 = Kf^-1 (-g_F), G = Kf^-1 A_F',
    (A_F G - eps I) dnu = A_F u0, dv_F = u0 - G dnu, dv = 0 on the active set; then the reference's epilogue (:396-430)."""
    cot, x, u, lams, nus, Q, A, lb, ub, rho = [t.double() if torch.is_tensor(t) else t for t in pt]
    B, n = x.shape[0], x.shape[1]
    m = 0 if A is None else A.shape[1]
    eps = 1e-8
    out = {k: [] for k in FT.GRADS}
    free = FT.free_set(pt, torch.float64)
    for b in range(B):
        F = free[b].nonzero().squeeze(1)
        nf = len(F)
        dv, dnu = torch.zeros(n, 1, dtype=torch.float64), torch.zeros(m, 1, dtype=torch.float64)
        if nf:
            Kf = Q[b][F][:, F] + eps * torch.eye(nf, dtype=torch.float64)
            u0 = torch.linalg.solve(Kf, -cot[b][F])
            if m:
                AF = A[b][:, F]
                G = torch.linalg.solve(Kf, AF.T)
                dnu = torch.linalg.solve(AF @ G - eps * torch.eye(m, dtype=torch.float64), AF @ u0)
                u0 = u0 - G @ dnu
            dv[F] = u0
        kkt = -cot[b] - Q[b] @ dv
        if m:
            kkt = kkt - A[b].T @ dnu
        rb = 1.0 if rho is None else float(rho[b]) if torch.is_tensor(rho) else float(rho)
        div = rb * u[b]
        div = torch.where(div == 0, torch.ones_like(div), div)
        dlam = kkt / div
        half = 0.5 * dv @ x[b].T
        out["dQ"].append(half + half.T)
        out["dp"].append(dv)
        out["dA"].append(dnu @ x[b].T + nus[b] @ dv.T if m else None)
        out["db"].append(-dnu if m else None)
        out["dlb"].append(dlam * lams[b, :n])
        out["dub"].append(-dlam * lams[b, n:])
    return {k: (None if v[0] is None else torch.stack(v)) for k, v in out.items()}


ORACLE_ROWS = [r["name"] for r in FT.ROWS if r["n"] <= 600]
ORACLE_BOUND = 1e-12


@pytest.mark.parametrize("name", ORACLE_ROWS)
def test_oracle_is_the_reduced_solve_on_the_free_set(name):
    """float64: the oracle's full (n + m) system (rows of the active set reduced to (rho + 1e-8) dv_i = 0) against the Schur
    complement on the free set, dv = 0 on the active set, the same epilogue.  Measured over these rows: at most 8.9e-15 of scale
    (dlb of chol_nf512_513_n576); the bound is two orders above that, 1e-12 of scale -- four orders tighter than the 1e-8 of scale
    a float32 budget of 1e-7 could still tell apart."""
    r = FT.ROW_BY_NAME[name]
    idx, pt = _sampled(r)
    full = FT.oracle(pt, torch.float64)
    red = _reduced(pt)
    for k in FT.GRADS:
        assert (full[k] is None) == (red[k] is None), k
        if full[k] is not None:
            e = float((full[k] - red[k]).abs().max()) / _scale(full[k])
            print(f"{name} {k}: full against reduced {e:.3e} of scale")
            assert e <= ORACLE_BOUND, (k, e)


def test_three_variables_by_hand():
    """Variable 0 active at its lower bound, 1 free, 2 active at its upper bound; Q couples them, no equality rows:
    dv = (0, -g1 / (q11 + 1e-8), 0), kkt = -g - Q dv, dlam = kkt / (rho u) (1 where u = 0), dlb = dlam lam_lo, dub = -dlam lam_hi."""
    Q = torch.tensor([[[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 2.0]]], dtype=torch.float64)
    g = torch.tensor([[[1.0], [2.0], [-3.0]]], dtype=torch.float64)
    lb = torch.tensor([[[0.0], [-1.0], [-4.0]]], dtype=torch.float64)
    ub = torch.tensor([[[1.0], [3.0], [2.0]]], dtype=torch.float64)
    x = torch.tensor([[[0.0], [0.5], [2.0]]], dtype=torch.float64)
    u = torch.tensor([[[-0.5], [0.0], [0.25]]], dtype=torch.float64)
    lams = torch.tensor([[[0.5], [0.0], [0.0], [0.0], [0.0], [0.25]]], dtype=torch.float64)
    for rho in (None, 0.7, torch.tensor([[[0.7]]], dtype=torch.float64)):
        rv = 1.0 if rho is None else 0.7
        dQ, dp, dA, db, dlb, dub, last = O.solve_box_qp_grad(g, x, u, lams, None, Q, None, lb, ub, rho)
        assert dA is None and db is None and last is None
        dv1 = -2.0 / (2.0 + 1e-8)
        dv = [0.0, dv1, 0.0]
        assert torch.allclose(dp[0, :, 0], torch.tensor(dv, dtype=torch.float64), rtol=1e-13, atol=0)
        xs = [0.0, 0.5, 2.0]
        for i in range(3):
            for j in range(3):
                assert abs(float(dQ[0, i, j]) - 0.5 * (dv[i] * xs[j] + xs[i] * dv[j])) <= 1e-13
        kkt = [-1.0 - 1.0 * dv1, -2.0 - 2.0 * dv1, 3.0 - 1.0 * dv1]
        dlam = [kkt[0] / (rv * -0.5), kkt[1] / 1.0, kkt[2] / (rv * 0.25)]
        want_lb = [dlam[0] * 0.5, 0.0, 0.0]
        want_ub = [0.0, 0.0, -dlam[2] * 0.25]
        assert torch.allclose(dlb[0, :, 0], torch.tensor(want_lb, dtype=torch.float64), rtol=1e-12, atol=0)
        assert torch.allclose(dub[0, :, 0], torch.tensor(want_ub, dtype=torch.float64), rtol=1e-12, atol=0)
        # ... x + u exactly ON a bound stays free (the strict comparisons of :360-365): variable 1 at its upper bound
        x2 = x.clone()
        x2[0, 1, 0] = 3.0
        dp2 = O.solve_box_qp_grad(g, x2, u, lams, None, Q, None, lb, ub, rho)[1]
        assert torch.allclose(dp2[0, :, 0], torch.tensor(dv, dtype=torch.float64), rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
def backward_knobs():
    return sorted(k for k in documented_knobs() if k.startswith("LQP_BWD_") or k in FT.BACKWARD_KNOBS_EXTRA)


def uncovered_knobs(rows):
    knobs = documented_knobs()
    forced = {k for r in rows for k, v in r["env"].items() if v != knobs.get(k)}
    return sorted(k for k in backward_knobs() if k not in FT.NOT_READ and k not in forced)


def uncovered_thresholds(rows):
    missing = []
    for what, (key, lo, hi) in FT.THRESHOLDS.items():
        vals = set().union(*[FT.threshold_values(key, r) for r in rows])
        if not (lo in vals and hi in vals):
            missing.append(what)
    return missing


LARGE_ROWS = {"chol_nfn_n1024", "chol_nf65_n1024", "chol_nf1_n1024", "chol_m16_nf600_n1024", "planner_n1025_m0", "lu_n1100_f64"}


def test_rows_cover_every_threshold_entry_rho_and_knob():
    knobs = documented_knobs()
    assert len(backward_knobs()) >= 10, backward_knobs()
    assert set(FT.NOT_READ) <= set(backward_knobs()) and all(FT.NOT_READ.values())
    assert len({r["name"] for r in FT.ROWS}) == len(FT.ROWS) >= 40
    for r in FT.ROWS:
        name = r["name"]
        assert set(r["env"]) <= set(knobs) and set(r["flip"] or {}) <= set(knobs), name
        assert r["dtype"] in ("f32", "f64") and r["entry"] in FT.ENTRIES and r["form"] in FT.FORMS and FT.rho_kind(r) in FT.RHOS, name
        assert r["q"] in ("sym", "nonsym", "indef") and T.batch(r, CUS) >= 1, name
        assert r["R"] <= T.R_MAX and r["F"] <= T.F_MAX, name
        if (r["R"], r["F"]) != (T.R_DEFAULT, T.F_DEFAULT) or r["same"]:
            assert r["why"] and "measured" in r["why"], (name, "a raised bar or a same-bits flip needs its measured reason")
        if r["dtype"] == "f64" or r["q"] == "nonsym":
            assert not FT.ran_chol(r) and r["form"] != "fallback", name       # (the Cholesky form is float32 on a symmetric Q)
        if FT.ran_chol(r):
            assert r["entry"] == r["form"] and r["n"] <= 1024 and r["m"] <= 16, name
        if r["entry"].endswith("_pre"):
            assert r["form"] == r["entry"], name
        assert isinstance(r["B"], int) and r["B"] <= 6 or (r["B"] == "cus + 3" and r["n"] == 130), name
        assert (r["n"] > 600) == (name in LARGE_ROWS), name
        if r["n"] >= 1000:
            assert r["B"] <= 2, name                                           # (the oracle's cost)
        for v in FT.nf_values(r):
            assert r["m"] == 0 or v == 0 or v >= r["m"] + 8, name              # (fewer free variables than equality rows: no truth)
    assert uncovered_knobs(FT.ROWS) == []
    assert uncovered_thresholds(FT.ROWS) == []
    assert {r["entry"] for r in FT.ROWS} == set(FT.ENTRIES)
    for entry in ("chol", "lu"):
        assert {FT.rho_kind(r) for r in FT.ROWS if r["entry"] == entry} == set(FT.RHOS), entry
    assert {FT.rho_kind(r) for r in FT.ROWS if r["entry"].endswith("_pre")} == set(FT.RHOS)
    assert {r["dtype"] for r in FT.ROWS if r["entry"] in ("lu", "lu_pre")} == {"f32", "f64"}
    assert "cus + 3" in {r["B"] for r in FT.ROWS}
    assert any(r["want"] and r["entry"] == "chol" and r["m"] > 0 for r in FT.ROWS) and any(r["want"] and r["entry"] == "chol_pre" for r in FT.ROWS)
    # the float16-pipe knobs sit where the look-ahead runs (2 to 7 blocks) and must bite
    for k in ("LQP_BWD_F16", "LQP_BWD_EQUIL", "LQP_SPD_F16"):
        rows = [r for r in FT.ROWS if k in r["env"]]
        assert rows and all(FT.ran_chol(r) and not r["same"] and {T.ks(v) for v in FT.nf_values(r)} <= set(range(2, 8)) for r in rows), k
    # every factor routine inside ONE launch, and the empty free set on every entry family
    assert any({1, 2, 7, 8, 9} <= FT.threshold_values("Kb", r) for r in FT.ROWS)
    assert {r["entry"] for r in FT.ROWS if 0 in FT.nf_values(r)} >= {"chol", "lu", "lu_pre"}
    assert {r["m"] for r in FT.ROWS if FT.nf_values(r) == {0} and r["entry"] == "chol"} == {0, 1}
    assert {r["m"] for r in FT.ROWS if FT.nf_values(r) == {0} and r["entry"] == "lu"} == {0, 1}
    assert {r["m"] for r in FT.ROWS if FT.ran_chol(r)} >= {0, 1, 2, 3, 16}


def test_coverage_check_fails_without_its_rows():
    """The coverage check is not vacuous: without the only row that forces a knob, or without one side of a threshold, it fails."""
    knob_rows = {}
    for r in FT.ROWS:
        for k in r["env"]:
            knob_rows.setdefault(k, []).append(r["name"])
    singles = [k for k, v in sorted(knob_rows.items()) if len(v) == 1]
    assert singles
    for only in singles:
        assert uncovered_knobs([r for r in FT.ROWS if r["name"] != knob_rows[only][0]]) == [only]
    for what, (key, lo, hi) in FT.THRESHOLDS.items():
        for side in (lo, hi):
            assert what in uncovered_thresholds([r for r in FT.ROWS if side not in FT.threshold_values(key, r)]), (what, side)


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator
SENS_ROWS = [r["name"] for r in FT.ROWS if r["dtype"] == "f32" and r["n"] <= 600]


def _first(mask):
    """(problem, variable) of the first True of a (B, n) mask, or None."""
    hit = mask.nonzero()
    return None if len(hit) == 0 else (int(hit[0, 0]), int(hit[0, 1]))


def _tie_to_active(args):
    x, u, lb, ub = args[1], args[2], args[7], args[8]
    free = ~(((x + u) > ub) | ((x + u) < lb)).squeeze(2)
    b, j = _first(free & ((x == ub) | (x == lb)).squeeze(2))
    args = list(args)
    args[2] = u.clone()
    args[2][b, j, 0] = 1.0 / 64 if x[b, j, 0] == ub[b, j, 0] else -1.0 / 64
    return args


def _negate_u(args):
    b, j = _first((args[2] != 0).squeeze(2))
    args = list(args)
    args[2] = args[2].clone()
    args[2][b, j, 0] = -args[2][b, j, 0]
    return args


def _ignore_rho(args):
    return list(args[:9]) + [1.0]


def _perturb_q(args):
    args = list(args)
    args[5] = T.perturb_last_block(args[5])
    return args


def _wrong_sign(t):
    return dict(t, dlb=-t["dlb"], dub=-t["dub"])


@pytest.mark.parametrize("name", SENS_ROWS)
def test_comparator_sees_errors(name):
    """With the oracle's float32 backward standing in for the GPU's the row passes at its own R and F; it fails with one free
    variable that sits on its bound taken for active, with dlb / dub of the wrong sign, with rho taken as 1, with the last diagonal
    64-block of Q scaled by 1 + 1e-4, and with u of one active variable negated -- each wherever the row's point has what the error
    needs (a tie, an active variable, a rho other than 1, a free variable)."""
    r = FT.ROW_BY_NAME[name]
    idx, pt = _sampled(r)
    t64 = FT.oracle(pt, torch.float64)
    t32 = FT.oracle(pt, torch.float32)
    ok = FT.compare(r, t32, t32, t64)
    assert all(rec["ok"] for rec in ok.values()) and {"dQ", "dp", "dlb", "dub"} <= set(ok), ok
    free = FT.free_set(pt, torch.float32)
    has_tie = _first(free & ((pt[1] == pt[8]) | (pt[1] == pt[7])).squeeze(2)) is not None
    has_active = not bool(free.all())
    has_free = bool(free.any())
    wrong = {}
    if has_tie:
        wrong["a tie taken for active"] = FT.oracle(pt, torch.float32, hook=_tie_to_active)
    if has_active:
        wrong["dlb / dub of the wrong sign"] = _wrong_sign(t32)
        wrong["u of an active variable negated"] = FT.oracle(pt, torch.float32, hook=_negate_u)
        if r["rho"] is not None:
            wrong["rho ignored"] = FT.oracle(pt, torch.float32, hook=_ignore_rho)
    if has_free:
        wrong["one tile of Q"] = FT.oracle(pt, torch.float32, hook=_perturb_q)
    assert wrong, name
    if 3 < min(FT.nf_values(r)) and max(FT.nf_values(r)) < r["n"]:
        assert len(wrong) == (5 if r["rho"] is not None else 4), sorted(wrong)
    for what, w in wrong.items():
        res = FT.compare(r, w, t32, t64)
        assert not all(rec["ok"] for rec in res.values()), (what, {k: (v["err"], v["bar"]) for k, v in res.items()})
