"""CPU checks of tests/direct_table.py and of the oracle functions it takes for the truth: the rows sit on both sides of every edge
of the code behind the direct entry points (EDGES; without the rows of one side the check fails), the oracle is the dense algebra
written out, every float32 budget is non-zero where the truth is and the matrices are well conditioned, and the comparator of
tests/test_gpu_direct.py sees a one-tile error of M, two exchanged pivots and a no-bound layer that kept rho = 1."""
import pytest
import torch

import direct_table as DT
import tier_table as T
from oracle import boxqp_oracle as O
from test_tier_table import documented_knobs

NAMES = [r["name"] for r in DT.ROWS if r["singular"] is None]
_cache = {}


def _row(name):
    """(row, inputs, t64, t32 or None), built once per row and left unchanged."""
    if name not in _cache:
        r = DT.ROW_BY_NAME[name]
        inp = DT.inputs(r)
        _cache[name] = (r, inp, DT.truth(r, inp, torch.float64), DT.truth(r, inp, torch.float32) if r["dtype"] == "f32" else None)
    return _cache[name]


def _scale(t):
    return max(1.0, float(t.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the table: both sides of every edge
def K(r):
    return T.ks(r["N"])


def _plain(r):
    return not r["env"] and r["factor"] == "hip"


EDGES = {}            # what -> (rows of the lower side, rows of the upper side), as predicates


def edge(what, family, dtypes, lo, hi):
    for dt in dtypes:
        fam = lambda r, dt=dt: r["family"] == family and r["dtype"] == dt and r["singular"] is None
        EDGES[f"{family} {dt}: {what}"] = ((lambda r, fam=fam: fam(r) and lo(r)), (lambda r, fam=fam: fam(r) and hi(r)))


BOTH = ("f32", "f64")
# k_pack / k_packed_solve (csrc/lqp_trsv.hpp, csrc/lqp_boxqp.hpp), per dtype where the constants differ
edge("K 1 | 2", "solve", BOTH, lambda r: K(r) == 1, lambda r: K(r) == 2)
edge("K 2 | 3", "solve", BOTH, lambda r: K(r) == 2, lambda r: K(r) == 3)
edge("N % 4 zero (vector loads) | non-zero (scalar loads)", "solve", BOTH, lambda r: r["N"] % 4 == 0 and r["N"] > 4, lambda r: r["N"] % 4 != 0 and r["N"] > 4)
edge("N % 64 zero | non-zero (the interchange walk over a partial block)", "solve", BOTH, lambda r: r["N"] % 64 == 0, lambda r: r["N"] % 64 != 0 and K(r) > 1)
edge("ring exact | padded, nrhs > 1", "solve", BOTH, lambda r: DT.ring_exact(r) and DT.nrhs(r) > 1 and K(r) > 1,
     lambda r: not DT.ring_exact(r) and DT.nrhs(r) > 1 and K(r) > 1)
edge("staging groups 1 | 2", "solve", BOTH, lambda r: DT.pack_groups(r) == 1 and K(r) > 1, lambda r: DT.pack_groups(r) == 2)
edge("B 128 | 129 (two workgroups per factor | one)", "solve", BOTH, lambda r: r["B"] <= 128 and r["N"] in (65, 130) and not r["env"], lambda r: r["B"] == 129)
edge("LQP_SPLIT2 default | 0", "solve", BOTH, lambda r: DT.pack_split(r) and r["N"] in (65, 130), lambda r: r["env"].get("LQP_SPLIT2") == "0" and r["same"])
edge("rhs (B,N) | (B,N,1)", "solve", BOTH, lambda r: r["rhs"] == "2d", lambda r: r["rhs"] == "k1" and r["N"] > 1)
edge("nrhs 1 | 3", "solve", BOTH, lambda r: r["rhs"] == "k1" and K(r) > 1, lambda r: r["rhs"] == "k3" and K(r) > 1)
edge("nrhs 3 | 17", "solve", BOTH, lambda r: r["rhs"] == "k3", lambda r: r["rhs"] == "k17")
edge("rhs contiguous | a transposed view", "solve", BOTH, lambda r: r["rhs"] == "k3", lambda r: r["rhs"] == "k3t")
edge("rhs forms at N = 65 | at N = 200", "solve", BOTH, lambda r: r["N"] == 65 and r["rhs"] in ("2d", "k17", "k3t"), lambda r: r["N"] == 200 and r["rhs"] in ("2d", "k17", "k3t"))
edge("factor by lu_factor | by LAPACK", "solve", BOTH, lambda r: r["factor"] == "hip" and r["N"] in (65, 130, 513), lambda r: r["factor"] == "torch")
edge("N 1 | > 1", "solve", BOTH, lambda r: r["N"] == 1, lambda r: r["N"] > 1)
edge("N 512 | 513", "solve", BOTH, lambda r: r["N"] == 512, lambda r: r["N"] == 513 and _plain(r))
edge("N 1024 | 1025", "solve", BOTH, lambda r: r["N"] == 1024, lambda r: r["N"] == 1025)
EDGES["solve: N 2048 | 2049"] = (lambda r: r["family"] == "solve" and r["N"] == 2048, lambda r: r["family"] == "solve" and r["N"] == 2049)
EDGES["solve f32: N 2049 | 4096 (the largest)"] = (lambda r: r["family"] == "solve" and r["N"] == 2049, lambda r: r["family"] == "solve" and r["N"] == 4096)
# the LU layer
edge("rhs (B,N) | (B,N,3)", "lulayer", BOTH, lambda r: r["rhs"] == "2d", lambda r: r["rhs"] == "k3")
edge("N 65 | 200", "lulayer", BOTH, lambda r: r["N"] == 65, lambda r: r["N"] == 200)
edge("symmetric | non-symmetric M", "lulayer", BOTH, lambda r: r["q"] == "sym", lambda r: r["q"] == "nonsym")
# k_kkt_build / k_kkt_unpack / k_outer_grads (csrc/lqp_boxqp.hpp, csrc/lqp_amd.hip)
edge("n 1 | > 1", "eqcon", BOTH, lambda r: r["n"] == 1, lambda r: r["n"] > 1)
edge("N 64 | 65 (the padded workspace gains a block)", "eqcon", BOTH, lambda r: r["N"] == 64, lambda r: r["N"] == 65)
edge("m < n | m = n", "eqcon", BOTH, lambda r: r["m"] < r["n"], lambda r: r["m"] == r["n"])
edge("m 16 | 17 (a second trip of the loops over LQP_NW)", "eqcon", BOTH, lambda r: r["m"] <= 16, lambda r: r["m"] >= 17)
edge("m 64 | 65 (a second trip of the loops over 64)", "eqcon", BOTH, lambda r: r["m"] <= 64, lambda r: r["m"] >= 65)
edge("N 512 | 513", "eqcon", BOTH, lambda r: r["N"] == 512, lambda r: r["N"] == 513)
edge("N <= 1024 | 1025", "eqcon", ("f32",), lambda r: r["N"] <= 1024, lambda r: r["N"] == 1025)
edge("n 1 | > 1", "uncon", BOTH, lambda r: r["n"] == 1, lambda r: r["n"] > 1)
edge("n 64 | 65", "uncon", BOTH, lambda r: r["n"] == 64, lambda r: r["n"] == 65)
edge("n <= 512 | 513", "uncon", BOTH, lambda r: 65 < r["n"] <= 512, lambda r: r["n"] == 513)
EDGES["optnet: f32 | f64"] = (lambda r: r["family"] == "optnet" and r["dtype"] == "f32", lambda r: r["family"] == "optnet" and r["dtype"] == "f64")
# the no-bound layer: one side per LU tier plan_forward can give such a batch (csrc/lqp_amd.hip)
_auto = lambda r: "launch_mode" not in r["ctl"] and r["ctl"].get("sync", True) and r["ctl"].get("scale", True)
edge("dense on two workgroups (N <= 256) | on W workgroups", "layer0", BOTH, lambda r: _auto(r) and r["N"] <= 256, lambda r: _auto(r) and 256 < r["N"] <= 1024)
edge("dense | the one-workgroup loop (launch_mode = 1)", "layer0", ("f32",), lambda r: _auto(r) and r["N"] <= 1024, lambda r: r["ctl"].get("launch_mode") == 1)
edge("N <= 1024 | the wide LU", "layer0", ("f32",), lambda r: _auto(r) and r["N"] <= 1024, lambda r: _auto(r) and r["N"] > 1024)
edge("scale True | False", "layer0", ("f32",), lambda r: r["N"] == 259 and _auto(r), lambda r: r["ctl"].get("scale") is False)
edge("m 0 | > 0", "layer0", ("f32",), lambda r: r["m"] == 0 and r["N"] <= 256, lambda r: r["m"] > 0 and r["N"] <= 256)
edge("sync True | False", "layer0", ("f32",), lambda r: r["N"] == 259 and _auto(r), lambda r: r["ctl"].get("sync") is False)
EDGES["layer0: f32 | f64"] = (lambda r: r["family"] == "layer0" and r["dtype"] == "f32", lambda r: r["family"] == "layer0" and r["dtype"] == "f64")


def uncovered_edges(rows):
    return sorted(what for what, (lo, hi) in EDGES.items() if not (any(lo(r) for r in rows) and any(hi(r) for r in rows)))


def test_rows_sit_on_both_sides_of_every_edge():
    knobs = documented_knobs()
    assert len(EDGES) >= 60
    assert uncovered_edges(DT.ROWS) == []
    assert {r["family"] for r in DT.ROWS} == set(DT.FAMILIES)
    assert {r["tier"] for r in DT.ROWS if r["family"] == "layer0" and r["dtype"] == "f32"} == set(DT.TIERS)
    for r in DT.ROWS:
        name = r["name"]
        assert r["dtype"] in BOTH and r["rhs"] in DT.RHS_FORMS and r["factor"] in ("hip", "torch") and r["q"] in ("sym", "nonsym"), name
        assert set(r["env"]) <= set(knobs), name
        assert r["N"] == r["n"] + r["m"] <= (4096 if r["dtype"] == "f32" else 2048), name
        assert r["R"] <= T.R_MAX and r["F"] <= T.F_MAX, name
        if (r["R"], r["F"]) != (T.R_DEFAULT, T.F_DEFAULT):
            assert r["why"] and "measured" in r["why"], (name, "a raised bar needs its measured ratio")
        if r["same"]:
            assert r["env"] and r["why"], name
        if r["N"] > 1024:
            assert r["B"] <= 2, name                     # (the oracle's cost)
        assert (r["tier"] in DT.TIERS) == (r["family"] == "layer0"), name
        if r["j"]:
            assert r["m"] == r["n"] and r["why"], name
    # the largest sizes once each; the four ring rows: exact and padded in either dtype, three right-hand sides
    for N in (2049, 4096):
        assert len([r for r in DT.ROWS if r["N"] == N]) == 1, N
    ring = {(r["dtype"], r["N"]): (K(r), DT.ring_exact(r)) for r in DT.ROWS if r["name"].startswith("solve_ring_")}
    assert ring == {("f32", 448): (7, True), ("f32", 192): (3, False), ("f64", 192): (3, True), ("f64", 256): (4, False)}
    assert all(DT.nrhs(r) == 3 for r in DT.ROWS if r["name"].startswith("solve_ring_"))
    assert {("f32", 513), ("f64", 257)} <= {(r["dtype"], r["N"]) for r in DT.ROWS if r["family"] == "solve" and DT.pack_groups(r) == 2 and _plain(r)}
    sing = [r for r in DT.ROWS if r["singular"] is not None]
    assert {r["dtype"] for r in sing} == set(BOTH) and all(r["family"] == "eqcon" and r["B"] == 4 and r["singular"][0] == 2 for r in sing)


def test_coverage_check_fails_without_its_rows():
    """The coverage check is not vacuous: without the rows of either side of an edge it names that edge."""
    for what, sides in EDGES.items():
        for side in sides:
            assert what in uncovered_edges([r for r in DT.ROWS if not side(r)]), what


# ---------------------------------------------------------------------------------------------------------------------------------
# the truth, written out by hand (float64)
def _kkt_solve(Q, A, top, bot, ridge=0.0):
    """Literal dense solve of [[Q, A'], [A, 0]] (+ ridge I) [x; nu] = [top; bot] through the explicit inverse."""
    B, n = Q.shape[0], Q.shape[1]
    m = 0 if A is None else A.shape[1]
    M = torch.zeros(B, n + m, n + m, dtype=torch.float64)
    M[:, :n, :n] = Q
    if m:
        M[:, n:, :n] = A
        M[:, :n, n:] = A.transpose(1, 2)
    M = M + ridge * torch.eye(n + m, dtype=torch.float64)
    v = torch.linalg.inv(M) @ (top if m == 0 else torch.cat((top, bot), 1))
    return v[:, :n], (v[:, n:] if m else None)


def _qp_grads(dx, dnu, x, nus):
    out = dict(dQ=0.5 * (dx @ x.transpose(1, 2) + x @ dx.transpose(1, 2)), dp=dx)
    if dnu is not None:
        out.update(dA=dnu @ x.transpose(1, 2) + nus @ dx.transpose(1, 2), db=-dnu)
    return out


def _close(name, got, want):
    assert set(want) <= set(got), (name, sorted(got), sorted(want))
    for k, w in want.items():
        e = float((DT.as3(got[k]) - DT.as3(w)).abs().max()) / _scale(w)
        print(f"{name} {k}: oracle against the algebra by hand {e:.3e} of scale")
        assert e <= 1e-12, (name, k, e)


BY_HAND = ("solve_n65_k3_f64", "lulayer_nonsym_n130_f64", "eqcon_n60_m5_f64", "uncon_n65_f64", "optnet_n70_m2_f64", "layer0_noscale_n257_m2_f32")


@pytest.mark.parametrize("name", BY_HAND)
def test_oracle_is_the_algebra_by_hand(name):
    """One small row per family, float64: x, nu = solve([[Q, A'], [A, 0]], [-p; b]); dx, dnu = the same solve of [-g; 0];
    dQ = (dx x' + x dx') / 2, dp = dx, dA = dnu x' + nus dx', db = -dnu; the LU layer's dA = dx x', db = -dx with dx = solve(M, -g)
    -- with M itself, also where M is not symmetric.  The no-bound layer without scaling is the same solve; its KKT backward the same
    gradients; its fixed-point backward the same with the reference's 1e-8 ridge on the whole diagonal, dlb = dub = 0."""
    r, inp, t64, _ = _row(name)
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in inp.items() if k != "point"}
    Q, p, A, b, M, cot = (d[k] for k in ("Q", "p", "A", "b", "M", "cot"))
    fam = r["family"]
    assert {DT.ROW_BY_NAME[n]["family"] for n in BY_HAND} == set(DT.FAMILIES)
    if fam in ("solve", "lulayer"):
        Minv = torch.linalg.inv(M)
        x = Minv @ d["base"]
        want = dict(x=x)
        if fam == "lulayer":
            assert not torch.equal(M, M.transpose(1, 2))
            dx = Minv @ (-d["gbase"])
            want.update(dA=dx @ x.transpose(1, 2), db=-dx)
        return _close(name, t64, want)
    pt = {k: (None if v is None else v.double()) for k, v in DT.point(r, inp).items()} if fam != "optnet" else None
    x, nus = _kkt_solve(Q, A, -p, b)
    dx, dnu = _kkt_solve(Q, A, -cot, None if A is None else torch.zeros_like(b))
    at = dict(x=x, nus=nus) if fam == "optnet" else pt
    if fam != "layer0":
        want = dict(x=x, **_qp_grads(dx, dnu, at["x"], at["nus"]))
        if nus is not None:
            want["nus"] = nus
        assert set(want) == set(t64)
        return _close(name, t64, want)
    zero = torch.zeros_like(p)
    want = dict(x=x, z=x, nus=nus, u=zero, lams=torch.cat((zero, zero), 1))
    want.update({f"kkt.{k}": v for k, v in _qp_grads(dx, dnu, x, nus).items()})
    dxr, dnur = _kkt_solve(Q, A, -cot, torch.zeros_like(b), ridge=1e-8)
    want.update({f"fp.{k}": v for k, v in _qp_grads(dxr, dnur, x, nus).items()})
    want.update({f"direct.{k}": v for k, v in _qp_grads(dxr, dnur, pt["x"], pt["nus"]).items()})
    want.update({"direct.dlb": zero, "direct.dub": zero})
    assert set(want) == set(t64)
    _close(name, t64, want)
    # (the ridge is what sets the fixed-point backward apart from the equality-constrained gradient: each entry has its own oracle)
    assert float((t64["fp.dQ"] - t64["kkt.dQ"]).abs().max()) > 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------
# the budgets
@pytest.mark.parametrize("name", NAMES)
def test_budget_is_usable(name):
    """|t32 - t64| > 0 for every output of a float32 row whose truth is not identically zero (the bar is the budget's, not F's
    alone), every truth finite, and cond(M) <= 1e4 for every row up to N = 1100 (above, the SVD costs minutes)."""
    r, inp, t64, t32 = _row(name)
    for k, v in t64.items():
        assert bool(torch.isfinite(v).all()), k
    if t32 is not None:
        assert set(t32) == set(t64)
        for k in t64:
            e32 = float((t32[k].double() - t64[k]).abs().max())
            if bool(t64[k].any()):
                assert e32 > 0.0, k
                assert e32 <= 1e-4 * _scale(t64[k]), (k, e32)
            else:
                assert e32 == 0.0 and k in ("u", "lams", "direct.dlb", "direct.dub"), k
    if r["N"] <= 1100:
        cond = float(torch.linalg.cond(inp["M"].double()).max())
        print(f"{name}: cond(M) {cond:.3g}")
        assert cond <= 1e4, cond


def test_singular_rows_have_an_exactly_zero_pivot():
    for r in DT.ROWS:
        if r["singular"] is None:
            continue
        inp = DT.inputs(r)
        i, k = r["singular"]
        assert not bool(inp["A"][i, k].any()) and not bool(inp["M"][i, r["n"] + k].any())
        info = torch.linalg.lu_factor_ex(inp["M"])[2]
        assert [int(v > 0) for v in info] == [int(j == i) for j in range(r["B"])], info


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator
def _perturb_M(r):
    """hook: the last (partial) diagonal 64-block of M scaled by 1 + 1e-4, and Q, A taken back out of it."""
    def hook(d):
        n = r["n"]
        M = T.perturb_last_block(d["M"])
        d = dict(d, M=M, Q=M[:, :n, :n].contiguous())
        if r["m"]:
            d["A"] = M[:, n:, :n].contiguous()
        return d
    return hook


def _row_order(piv):
    """The row order the interchanges piv (LAPACK's, 1-based, applied in sequence) leave."""
    order = list(range(len(piv)))
    for i, t in enumerate(piv):
        order[i], order[t - 1] = order[t - 1], order[i]
    return order


def _exchanged_pivots(r, inp):
    """The float32 solve of the row with two pivots of the last 64-block exchanged: the first two entries of the pivot vector there
    whose exchange leaves another row order, in every problem."""
    M, base = inp["M"].float(), inp["base"].float()
    LU, piv = torch.linalg.lu_factor(M)
    piv = piv.clone()
    N = r["N"]
    s = ((N - 1) // 64) * 64
    assert N - s >= 2
    for bi in range(M.shape[0]):
        was = piv[bi].tolist()

        def swapped(j, k):
            new = list(was)
            new[j], new[k] = was[k], was[j]
            return new
        pair = next(((j, k) for j in range(s, N) for k in range(j + 1, N) if _row_order(swapped(j, k)) != _row_order(was)), None)
        assert pair is not None, (r["name"], bi, "no exchange of two pivots of the last block changes the row order")
        piv[bi] = torch.tensor(swapped(*pair), dtype=piv.dtype)
    return torch.linalg.lu_solve(LU, piv, base)


def _layer_with_rho_one(r, inp, t32):
    """What the layer would give had the no-bound batch kept rho = 1 (float32, no scaling): one ADMM x-update from z = u = 0 is
    x = solve([[Q + I, A'], [A, 0]], [-p; b]); the gradients are then taken at that x."""
    Q, p, A, b, cot = (inp[k].float() for k in ("Q", "p", "A", "b", "cot"))
    sol = O.solve_qp_eqcon(Q + torch.eye(r["n"]), p, A, b)
    lb, ub = DT._unbounded(p)
    zero = torch.zeros_like(p)
    g = O.solve_box_qp_grad(cot, sol["x"], zero, torch.cat((zero, zero), 1), sol["nus"], Q, A, lb, ub, 1)
    out = dict(t32, x=sol["x"], z=sol["x"], nus=sol["nus"])
    out.update({f"fp.{k}": v for k, v in zip(("dQ", "dp", "dA", "db"), g)})
    return out


SENS = {"solve_n200_k3_f32": ("tile", "pivots"), "lulayer_n200_k3_f32": ("tile", "pivots"), "eqcon_n100_m17_f32": ("tile",),
        "layer0_noscale_n257_m2_f32": ("tile", "rho")}


@pytest.mark.parametrize("name", sorted(SENS))
def test_comparator_sees_errors(name):
    """With the oracle's float32 result standing in for the GPU's the row passes at its own R and F; it fails with the last diagonal
    64-block of M scaled by 1 + 1e-4, with two pivots of the last block exchanged in the solve, and with the no-bound layer solved
    and differentiated at rho = 1.  (The rho ARGUMENT of the fixed-point backward cannot be seen on such a batch -- every variable
    is free and u = 0, so rho multiplies zeros and the guard div == 0 -> 1 takes the division: checked here bit for bit; what a
    kept rho changes is the solution.)"""
    r, inp, t64, t32 = _row(name)
    ok = DT.compare(r, t32, t32, t64)
    assert all(rec["ok"] for rec in ok.values()) and set(ok) == set(t64), ok
    wrong = {}
    if "tile" in SENS[name]:
        wrong["one tile of M"] = DT.truth(r, inp, torch.float32, hook=_perturb_M(r))
    if "pivots" in SENS[name]:
        wrong["two pivots exchanged"] = dict(t32, x=_exchanged_pivots(r, inp))
    if "rho" in SENS[name]:
        wrong["rho = 1 kept"] = _layer_with_rho_one(r, inp, t32)
        pt = DT.point(r, inp)
        a = [inp["cot"], pt["x"], pt["u"], pt["lams"], pt["nus"], inp["Q"], inp["A"], *DT._unbounded(inp["p"])]
        g0, g1 = O.solve_box_qp_grad(*a, 0), O.solve_box_qp_grad(*a, 1)
        assert all(torch.equal(u, v) for u, v in zip(g0[:6], g1[:6]))
    assert len(wrong) == len(SENS[name])
    for what, w in wrong.items():
        res = DT.compare(r, w, t32, t64)
        assert not all(rec["ok"] for rec in res.values()), (what, {k: (v["err"], v["bar"]) for k, v in res.items()})
