"""CPU checks of tests/unroll_table.py: the rows force every unroll knob and hold both sides of every boundary of the unroll backward's
selection code; every row's clamp decisions are settled (the unrolled gradient is discontinuous where x_k + u_k crosses a bound: a
row whose decisions float32 does not settle tests nothing); the comparator of tests/test_gpu_unroll.py sees a tape one iteration
short, one flipped clamp decision and a one-tile error of Q; and the oracle's tape agrees with the library's own restatement of
the reference's taped loop (lqp_py_amd.unrolled._eager_unrolled) in float64."""
import pytest
import torch

import tier_table as T
import unroll_table as U
from oracle import boxqp_oracle as O
from test_tier_table import documented_knobs

CUS = 256


def uncovered_knobs(rows):
    forced = {(k, v) for r in rows for k, v in r["env"].items()}
    return sorted(U.FORCED - forced)


def uncovered_thresholds(rows):
    missing = []
    for what, (key, lo, hi, flt) in U.THRESHOLDS.items():
        vals = {U.value(r, key) for r in rows if U.FILTERS[flt](r)}
        if lo not in vals or hi not in vals:
            missing.append(what)
    return missing


def test_rows_cover_every_unroll_knob_and_boundary():
    knobs = documented_knobs()
    unroll_knobs = {k for k in knobs if k.startswith("LQP_UNROLL_")}
    assert unroll_knobs == set(U.KNOBS) == {k for k, _ in U.FORCED}, "docs/KNOBS.md and unroll_table.KNOBS disagree"
    for k in U.KNOBS:
        assert "tests/unroll_table.py" in T.NOT_A_TIER[k], k
    for r in U.ROWS:
        assert set(r["env"]) <= set(U.KNOBS), r["name"]
        assert r["dtype"] in ("f32", "f64") and 0 < r["K"] <= T.K_EVENTS and 0 <= r["j"] < 16, r["name"]
        if r["K"] != (T.K_EVENTS if r["exp"]["n_factor"] > 1 else T.K_DEFAULT):
            assert r["why"], (r["name"], "a K of its own needs its reason")
        assert r["R"] <= T.R_MAX and r["F"] <= T.F_MAX, r["name"]
        if (r["R"], r["F"]) != (T.R_DEFAULT, T.F_DEFAULT):
            assert r["why"], (r["name"], "a raised bar needs its reason")
        assert set(r["exp"]) == {"ub", "us", "linsolve_used", "n_factor"}, r["name"]
        if r["exp"]["n_factor"] > 1:
            assert r["ctl"].get("rho") in (0.01, 100.0) and r["family"] in ("ev32", "ev64", "taped"), r["name"]
        if r["dtype"] == "f64":
            assert r["exp"]["linsolve_used"] == 1, r["name"]
        if r["family"] in ("one", "split", "big"):
            n, split = r["n"], r["split"]
            assert r["dtype"] == "f32" and r["m"] <= U.SPD_MAXM and n <= 1024 and "linsolve" not in r["ctl"], r["name"]
            assert (r["family"] == "big") == (n > 512), r["name"]
            if r["family"] == "split":
                assert U.ks(n) >= 5 and r["B"] != "cus//2 + 1" and r["env"].get("LQP_UNROLL_SPLIT") != "0", r["name"]
            if 128 < n <= 512 and not r["env"]:
                assert split == (r["family"] == "split"), (r["name"], "every unforced row says which sweep it expects")
        if r["n"] + r["m"] >= 2048:
            assert T.batch(r, CUS) == 1, r["name"]
    assert uncovered_knobs(U.ROWS) == []
    assert uncovered_thresholds(U.ROWS) == []
    # the control's variants of the scaling chain, the event tapes' variants
    ctls = [r["ctl"] for r in U.ROWS]
    assert any(c.get("scale") is False for c in ctls) and any(c.get("beta") == "tensor" for c in ctls)
    assert any(isinstance(c.get("beta"), float) for c in ctls) and any(c.get("rho") == 0.5 for c in ctls)
    ev64 = [r for r in U.ROWS if r["family"] == "ev64"]
    assert {r["ctl"]["rho"] for r in ev64} == {0.01, 100.0} and {r["m"] > 0 for r in ev64} == {True, False}
    assert {r["ctl"].get("scale", True) for r in ev64} == {True, False}
    ev32 = [r for r in U.ROWS if r["family"] == "ev32"]
    assert {r["ctl"]["rho"] for r in ev32} == {0.01, 100.0}
    assert {513, 576, 700, 1000, 1023, 1024} <= {r["n"] for r in U.ROWS if r["family"] == "big"}
    assert {1, 31, 64, 65, 128, 129} <= {r["n"] for r in U.ROWS if r["family"] == "one"}
    assert {60, 256, 257, 450} <= {r["n"] for r in U.ROWS if r["family"] == "lu64"}


def test_coverage_check_fails_without_its_rows():
    """The coverage check is not vacuous: without the rows that force a knob value, or without one side of a boundary, it fails."""
    for k, v in sorted(U.FORCED):
        assert uncovered_knobs([r for r in U.ROWS if r["env"].get(k) != v]) == [(k, v)]
    for what, (key, lo, hi, flt) in U.THRESHOLDS.items():
        for side in (lo, hi):
            rows = [r for r in U.ROWS if not (U.FILTERS[flt](r) and U.value(r, key) == side)]
            assert what in uncovered_thresholds(rows), (what, side)


@pytest.mark.parametrize("name", [r["name"] for r in U.ROWS])
def test_clamp_decisions_are_settled(name):
    """At the row's recorded seed offset: float32 rows, every clamp gap of the float64 tape is at least R_MAX times the float32 tape's
    deviation there; float64 rows, at least a hundred times the 1e-9 the row is held to.  n_factor is the row's in both tapes, and
    every gradient of the truth is finite (infinite bounds included: oracle.boxqp_oracle._scale_bound)."""
    r = U.ROW_BY_NAME[name]
    inp, cot, t64, t32, tr64, tr32 = U.row_tapes(r, CUS)
    v = U.settled(r, tr64, tr32)
    print(f"{name}: settled {v:.4g} (needs {T.R_MAX if r['dtype'] == 'f32' else U.F64_SETTLED}), j = {r['j']}")
    assert U.settled_ok(r, v), (name, v)
    assert len(tr64["clamps"]) == r["K"] + 1
    assert t64["n_factor"] == r["exp"]["n_factor"] and (t32 is None or t32["n_factor"] == r["exp"]["n_factor"]), name
    for t in (t64, t32):
        if t is not None:
            assert all(bool(torch.isfinite(g).all()) for g in t.values() if torch.is_tensor(g)), name
    tie = U.tie_mask(inp)
    assert r["n"] < 6 or bool(tie.any()) and bool(torch.isinf(inp[4]).any()) and bool(torch.isinf(inp[5]).any())


SENS_ROWS = ["one_n65_m0", "one_n129_m2", "split_n257_m1", "split_n321_m0", "noscale_n330", "lu32_m17_n200", "ev32_grow_n330",
             "ev32_shrink_n330"]


@pytest.mark.parametrize("name", SENS_ROWS)
def test_comparator_sees_a_wrong_tape(name):
    """With the oracle's float32 tape standing in for the GPU the row passes; it fails, at the row's own R and F, against (a) a tape
    one iteration short, (b) one clamp decision flipped (the lower bound closest below x_k + u_k at the last clamp that reaches x moved above it
    by its gap), (c) the last diagonal 64-block of Q scaled by 1 + 1e-4."""
    r = U.ROW_BY_NAME[name]
    inp, cot, t64, t32, tr64, tr32 = U.row_tapes(r, CUS)
    B = T.batch(r, CUS)
    idx = T.sample(B)
    tie = U.tie_mask(inp)
    ok = U.judge(r, t32, t32, t64, tie)
    assert all(rec["ok"] for rec in ok.values()) and {"x", "dQ", "dp", "dlb", "dub", "dlb+dub@tie"} <= set(ok), ok

    def fails(wrong, what):
        res = U.judge(r, wrong, t32, t64, tie)
        assert not all(rec["ok"] for rec in res.values()), (what, {k: (v["err"], v["bar"]) for k, v in res.items()})

    fails(U.tape(r, inp, torch.float32, cot, B, idx, K=r["K"] - 1)[0], "one iteration short")
    w, lbs, _ = tr64["clamps"][-2]                  # (the last clamp that reaches x: z_K of the last x-update)
    lbs = lbs.expand_as(w)
    gap = torch.where(torch.isfinite(lbs) & ~tie & (w > lbs), w - lbs, torch.full_like(w, float("inf")))      # (free above its lb)
    flat = int(gap.argmin())
    b_, i_ = flat // r["n"], flat % r["n"]
    D = lbs[b_, i_, 0] / inp[4][b_, i_, 0].double()                       # (scaled bound / bound = 1 / D_i)
    lb2 = inp[4].clone()
    lb2[b_, i_, 0] = lb2[b_, i_, 0] + (2 * gap[b_, i_, 0] / D).to(lb2.dtype)
    flipped, trf = U.tape(r, inp[:4] + (lb2, inp[5]), torch.float32, cot, B, idx)
    wf, lf, _ = trf["clamps"][-2]
    assert bool(wf[b_, i_, 0] < lf.expand_as(wf)[b_, i_, 0]), "the bumped bound did not flip the decision"
    fails(flipped, "one flipped clamp decision")
    fails(U.tape(r, (T.perturb_last_block(inp[0]),) + tuple(inp[1:]), torch.float32, cot, B, idx)[0], "one tile of Q")


class _CpuLU(torch.nn.Module):
    """CPU stand-in for the taped solve of lqp_py_amd.unrolled._eager_unrolled (the reference's lu_layer.py:5-58 with torch.linalg)."""

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, A, b, LU, piv):
            x = O.lu_solve(LU, piv, b)
            ctx.save_for_backward(LU, piv, x)
            return x

        @staticmethod
        def backward(ctx, g):
            LU, piv, x = ctx.saved_tensors
            dA, db = O.lu_layer_backward(LU, piv, x, g)
            return dA, db, None, None

    def __init__(self, A):
        super().__init__()
        with torch.no_grad():
            self.LU, self.piv = O.lu_factor(A)

    def forward(self, A, b):
        return self._Fn.apply(A, b, self.LU, self.piv)


def _eager64(r, inp, cot, B, idx):
    import lqp_py_amd.solve_box_qp_admm_torch as SB
    from lqp_py_amd.unrolled import _eager_unrolled
    leaves = [None if t is None else t.double().requires_grad_(True) for t in inp]
    ctl = U.make_control(r, B, idx, torch.float64)
    x = _eager_unrolled(*leaves, SB.resolve_control(ctl, r["n"]), True, True, solver_cls=_CpuLU)
    x.backward(cot.double())
    return dict(zip(U.GRADS, (None if t is None else t.grad for t in leaves)), x=x.detach())


@pytest.mark.parametrize("name", ["lu64_n60_m1", "one_n65_m0", "ev64_hi_noscale_n150_m2", "ev64_events0_n100_m1"])
def test_oracle_tape_agrees_with_the_eager_restatement(name):
    """The two statements of the reference's tape -- autograd through the oracle's loop (lu_factor / lu_solve differentiated by
    torch) and the library's _eager_unrolled with the reference's LU layer node on the CPU -- agree to 1e-12 of scale in float64:
    x, dQ (finite: an infinite bound carries no gradient into the scaling), dp, dA, db, and dlb, dub entry by entry (both are
    torch's clamps: the same split at lb == ub)."""
    r = U.ROW_BY_NAME[name]
    B = T.batch(r, CUS)
    idx = T.sample(B)
    inp = U.inputs(r, B, idx)
    cot = U.cotangent(r, B)[torch.tensor(idx)]
    t64, _ = U.tape(r, inp, torch.float64, cot, B, idx)
    e64 = _eager64(r, inp, cot, B, idx)
    for k in ("x",) + U.GRADS:
        if t64[k] is None:
            assert e64[k] is None
            continue
        assert bool(torch.isfinite(e64[k]).all()), (name, k)
        scale = max(1.0, float(t64[k].abs().max()))
        assert float((t64[k] - e64[k]).abs().max()) <= 1e-12 * scale, (name, k, float((t64[k] - e64[k]).abs().max()), scale)
