"""The KKT-system backward (backward='kkt'), as data (no GPU needed to import this module).

The backward is a function of (cot, x, lams, nus, Q, A, lb, ub) alone, so a row does not solve anything: `point` builds a synthetic
primal-dual point in float64 and rounds it ONCE to the row's dtype; the GPU call, the float32 oracle (the budget) and the float64
oracle (the truth, on the float32 values converted exactly) receive the same numbers.  tests/test_gpu_kkt.py runs every row on
the GPU against oracle.boxqp_oracle.solve_box_qp_grad_kkt with tier_table.compare (float32 rows |hip - t64| <= R |t32 - t64| + F scale,
float64 rows 1e-9 scale) and checks which form ran; tests/test_kkt_table.py checks, without a GPU, the oracle itself (golden g12,
full against reduced system, the bookkeeping of one-sided batches), the coverage of the rows and that the comparator sees errors.
tests/fp_table.py is this table's twin for the fixed-point backward (rows choose the size of the free set).

Row fields:
  name, n, m, dtype ("f32" | "f64"), B (int, or an expression of `cus`)
  entry    "chol":     SB._kkt_backward(..., flags=(any_lb, any_ub), linsolve=2) -- what the module calls behind the symmetric forward
           "lu":       L.torch_solve_box_qp_grad_kkt (the functional entry: it cannot know that Q is symmetric)
           "composed": the same with SB._KKT_NATIVE = False (torch ops around lqp_kkt_solve)
  sides    "both" | "lb" | "ub" | "none": which kinds of bound are finite anywhere in the batch
  q        "sym" | "nonsym" | "indef" (symmetric, one eigenvalue moved to -0.5 along interior variables: Q + diag(w) is not positive
           definite, the KKT matrix is regular)
  form     the form that must have run, by launch classes of _lib.profile(): FORMS[form] = (bwd_cholesky, lu_factor, bwd_epilogue)
  env      LQP_* overrides; flip / same / R / F / why as in tests/tier_table.py
  want     True: the row also calls with subsets of `want`; the outputs still asked for must keep their bits
"""
import math

import torch

import tier_table as T

GRADS = ("dQ", "dp", "dA", "db", "dlb", "dub")
PROF_CLASSES = ("bwd_cholesky", "lu_factor", "bwd_epilogue")
FORMS = {
    "chol": (1, 0, 1),          # blocked Cholesky of Q + diag(w), gradients in the epilogue
    "lu": (0, 1, 1),            # pivoted LU of the reduced KKT system, gradients in the epilogue
    "composed": (0, 1, 0),      # lqp_kkt_solve (the same LU chain) and torch ops
    "fallback": (1, 1, 2),      # the Cholesky attempt reports "not positive definite", the call repeats itself on the LU form
}
ENTRIES = ("chol", "lu", "composed")
SIDES = ("both", "lb", "ub", "none")


def row(name, n, m, B=3, dtype="f32", entry="chol", sides="both", env=None, q="sym", form=None, R=T.R_DEFAULT, F=T.F_DEFAULT,
        flip=None, same=False, want=False, why=None):
    env = dict(env or {})
    return dict(name=name, n=n, m=m, B=B, dtype=dtype, entry=entry, sides=sides, env=env, q=q, form=form or entry, R=R, F=F,
                flip=(dict(flip) if flip is not None else ({} if env else None)), same=same, want=want, why=why)


ROWS = [
    # ---------------- Cholesky form: every variable stays in the system, ceil(n / 64) blocks are factored ----------------
    row("chol_n1_m0", 1, 0, why="smallest system"),
    row("chol_n63_m1", 63, 1),
    row("chol_n64_m2", 64, 2, want=True),
    row("chol_n65_m3", 65, 3, why="two blocks; m = 3: the first four-right-hand-side instance"),
    row("chol_n128_m0", 128, 0),
    row("chol_n129_m16", 129, 16),
    row("chol_n448_m1", 448, 1, B=2, why="7 blocks: the largest look-ahead factorisation"),
    row("chol_n449_m2", 449, 2, B=2, why="8 blocks: wg_chol_factor"),
    row("chol_n512_m16", 512, 16, B=2),
    row("chol_n513_m1", 513, 1, B=2, why="9 blocks: wg_chol_factor_big"),
    row("chol_n1000_m3", 1000, 3, B=2),
    row("chol_n1024_m16", 1024, 16, B=2, why="16 blocks, m = 16: the largest LDS layout"),
    row("chol_n130_cus3", 130, 1, B="cus + 3", why="small_batch_split gives one slab"),
    row("chol_n130_B1", 130, 1, B=1),
    # ---------------- knobs ----------------
    row("chol_la0_n330", 330, 2, env={"LQP_BWD_LOOKAHEAD": "0"}, same=True,
        why="6 blocks: wg_chol_factor instead of wg_chol_factor_la, whose float32 build takes the same products in the same order "
            "inside every tile (its own comment): same bits (measured)"),
    row("chol_bwdf16off_n330", 330, 1, env={"LQP_BWD_F16": "0"}, same=True,
        why="backward='kkt' keeps float32 tile products (plan_backward), so the knob selects nothing here.  With the two-half float16 "
            "products of the look-ahead (2 to 7 blocks) dlb / dub = lam dx / slack, which divide the dx of a variable at its bound by "
            "1e-8, were measured at 4.5 to 19 times the float32 budget (rows n128_m0, n448_m1, n130, n200, n330; every other gradient "
            "within 2); without them at most 1.2: same bits (measured)"),
    row("chol_spdf16off_n449", 449, 3, B=2, env={"LQP_SPD_F16": "0"}, same=True,
        why="as LQP_BWD_F16, and 8 blocks run wg_chol_factor, which has no float16 products at all: same bits (measured)"),
    row("chol_equil0_n200", 200, 1, env={"LQP_BWD_EQUIL": "0"}, same=True,
        why="a power-of-two scaling commutes with every float32 operation of the factorisation and of the solves; it is there for the "
            "range of the float16 operands, which backward='kkt' does not take: same bits with weights from 1e-8 to 1e8, at the "
            "default R and F (measured: ratio at most 1.03)"),
    row("chol0_n200", 200, 2, env={"LQP_BWD_CHOL": "0"}, form="lu"),
    row("chol_early0_n200", 200, 1, env={"LQP_BWD_EARLY": "0"}, same=True,
        why="which launch stores the info words for the host does not touch the arithmetic (measured: same bits)"),
    row("chol_slabs1_n330", 330, 2, env={"LQP_EPI_SLABS": "1"}, same=True,
        why="the epilogue computes every row of dQ / dA whole, whichever slab it falls into (measured: same bits)"),
    # ---------------- one-sided and unbounded batches: the None pattern, the upper-only quirk ----------------
    row("chol_lb_n130", 130, 1, sides="lb"),
    row("chol_ub_n130", 130, 1, sides="ub"),
    row("chol_none_n130", 130, 1, sides="none"),
    row("chol_ub_n70_m0", 70, 0, sides="ub"),
    row("lu_lb_n130", 130, 1, entry="lu", sides="lb"),
    row("lu_ub_n130", 130, 1, entry="lu", sides="ub"),
    row("lu_none_n130", 130, 1, entry="lu", sides="none"),
    row("lu_ub_n70_m0", 70, 0, entry="lu", sides="ub"),
    # ---------------- LU form ----------------
    row("lu_n150_f64", 150, 2, dtype="f64", entry="lu"),
    row("lu_n257_m0_f64", 257, 0, dtype="f64", entry="lu"),
    row("lu_n450_f64", 450, 3, dtype="f64", entry="lu"),
    row("lu_n1100_f64", 1100, 1, B=1, dtype="f64", entry="lu"),
    row("planner_m17_n200", 200, 17, form="lu", why="m > 16: the planner itself leaves the Cholesky form"),
    row("planner_m16_n200", 200, 16, why="m = 16: the last m of the Cholesky form"),
    row("planner_n1025_m0", 1025, 0, B=2, form="lu", why="17 blocks: the planner itself leaves the Cholesky form"),
    row("lu_nonsym_n300", 300, 1, entry="lu", q="nonsym"),
    row("lu_split2off_n200", 200, 2, entry="lu", env={"LQP_SPLIT2": "0"}, same=True,
        why="the second workgroup per problem takes whole rows of the build and pack kernels: the same bits (measured)"),
    # ---------------- Q + diag(w) not positive definite: the Cholesky attempt gives up, the call repeats on the LU form ----------------
    row("fallback_indef_n200", 200, 1, q="indef", form="fallback"),
    # ---------------- composed from lqp_kkt_solve and torch ops: the baseline of the older tests ----------------
    row("composed_n130", 130, 1, entry="composed"),
    row("composed_n150_f64", 150, 2, dtype="f64", entry="composed"),
]

ROW_BY_NAME = {r["name"]: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS), "duplicate row names"

# the knobs of docs/KNOBS.md the backward's plan reads (plan_backward, enqueue_*): every LQP_BWD_* and these three
BACKWARD_KNOBS_EXTRA = ("LQP_EPI_SLABS", "LQP_SPLIT2", "LQP_SPD_F16")
# ... and those among them the KKT backward does not read, each with its reason
NOT_READ = {
    "LQP_BWD_FULL": "the KKT backward is the reduced system whatever the knob says (plan_backward: P.reduced)",
    "LQP_BWD_REFINE": "the refinement step belongs to the fixed-point backward's reduced LU form only (plan_backward: plan.refine)",
}

# block-count and size thresholds of plan_backward / k_bwd_chol_solve: (key, lower side, upper side); "K" = ceil(n / 64) of a Cholesky row
THRESHOLDS = {
    "K 1 | 2": ("K", 1, 2),
    "K 7 | 8 (look-ahead | wg_chol_factor)": ("K", 7, 8),
    "K 8 | 9 (wg_chol_factor | wg_chol_factor_big)": ("K", 8, 9),
    "n 1024 | 1025 (Cholesky form | LU)": ("n", 1024, 1025),
    "m 2 | 3 (two | four right-hand sides per round)": ("m_chol", 2, 3),
    "m 16 | 17 (Cholesky form | LU)": ("m", 16, 17),
}


def ran_chol(r):
    return FORMS[r["form"]][0] > 0


def threshold_value(key, r):
    """The row's value for a threshold key, or None when the row does not bear on it."""
    if key == "K":
        return T.ks(r["n"]) if r["form"] == "chol" else None
    if key == "m_chol":
        return r["m"] if r["form"] == "chol" else None
    return r[key] if r["entry"] == "chol" else None        # (n, m: what the planner decides on when asked for the Cholesky form)


def dtype_of(r):
    return torch.float32 if r["dtype"] == "f32" else torch.float64


def flags(r):
    return (r["sides"] in ("both", "lb"), r["sides"] in ("both", "ub"))


def none_pattern(r):
    """Which of GRADS the reference returns as None for this row."""
    any_lb, any_ub = flags(r)
    return dict(dQ=False, dp=False, dA=r["m"] == 0, db=r["m"] == 0, dlb=not any_lb, dub=not any_ub)


def _point(r, i, qcache):
    """Problem i of the row, float64: (cot, x, lams, nus, Q, A, lb, ub) with Q / A / bounds of tier_table._problem (some lb = -inf,
    some ub = +inf, a few lb == ub), the last variable interior, and each other variable one of: interior with lam = 0 (about 60 %) | exactly at lb, lam_lo in
    [0.01, 1] | exactly at ub, lam_hi in [0.01, 1] | 1e-6 inside lb, lam_lo = 1e-3 | exactly at ub with lam = 0 (both clamps act:
    w = 1) | fixed (lb == ub: both slacks clamped, lam_lo in [0.01, 1])."""
    n, m = r["n"], r["m"]
    Q, _, A, _, lb, ub = T._problem(r, i, qcache)
    inf = torch.full_like(lb, math.inf)
    if r["sides"] in ("ub", "none"):
        lb = -inf
    if r["sides"] in ("lb", "none"):
        ub = inf
    g = torch.Generator().manual_seed(T.seed_of(r) * 104729 + i)
    rnd = lambda: torch.rand(n, 1, generator=g, dtype=torch.float64)
    kind, frac, mult = rnd(), rnd(), 0.01 + 0.99 * rnd()
    kind[n - 1] = 0.0          # the last variable is interior: the last (partial) 64-block of Q, one entry at n = 64 k + 1, bears on dx
    flb, fub = torch.isfinite(lb), torch.isfinite(ub)
    lo = torch.where(flb, lb, torch.full_like(lb, -3.0))
    hi = torch.where(fub, ub, torch.full_like(ub, 3.0))
    x = lo + (hi - lo) * (0.1 + 0.8 * frac)
    lam_lo, lam_hi = torch.zeros_like(x), torch.zeros_like(x)
    at_lb = flb & (kind >= 0.60) & (kind < 0.72)
    at_ub = fub & (kind >= 0.72) & (kind < 0.84)
    near_lb = flb & (kind >= 0.84) & (kind < 0.90)
    at_ub0 = fub & (kind >= 0.90)
    fixed = flb & fub & (lb == ub)
    x = torch.where(at_lb, lb, x)
    lam_lo = torch.where(at_lb, mult, lam_lo)
    x = torch.where(at_ub | at_ub0, ub, x)
    lam_hi = torch.where(at_ub, mult, lam_hi)
    x = torch.where(near_lb, lb + 1e-6, x)
    lam_lo = torch.where(near_lb, torch.full_like(x, 1e-3), lam_lo)
    x = torch.where(fixed, lb, x)
    lam_lo = torch.where(fixed, mult, lam_lo)
    lam_hi = torch.where(fixed, torch.zeros_like(x), lam_hi)
    interior = ~(at_lb | at_ub | near_lb | at_ub0 | fixed)
    if r["q"] == "indef":
        v = torch.randn(n, 1, generator=g, dtype=torch.float64) * interior
        v = v / v.norm()
        Q = Q - (float(v.T @ Q @ v) + 0.5) * (v @ v.T)
    nus = torch.randn(m, 1, generator=g, dtype=torch.float64) if m else None
    cot = torch.randn(n, 1, generator=g, dtype=torch.float64)
    return cot, x, torch.cat((lam_lo, lam_hi), 0), nus, Q, A, lb, ub


def point(r, B, idx=None):
    """(cot, x, lams, nus, Q, A, lb, ub) of the batch -- or of the problems `idx` of it -- rounded once to the row's dtype."""
    dt = dtype_of(r)
    qcache = {}
    parts = [_point(r, i, qcache) for i in (range(B) if idx is None else idx)]
    return tuple(None if parts[0][k] is None else torch.stack([pt[k] for pt in parts]).to(dt) for k in range(8))


def oracle(pt, dtype, form="reduced", hook=None):
    """The CPU oracle's KKT backward of the point `pt` in `dtype` -> {name: tensor or None}.  `hook` (tests of the comparator) maps
    the converted arguments to wrong ones."""
    from oracle import boxqp_oracle as O
    args = [None if t is None else t.to(dtype) for t in pt]
    if hook is not None:
        args = hook(args)
    return dict(zip(GRADS, O.solve_box_qp_grad_kkt(*args, form=form)[:6]))


def compare(r, hip, t32, t64):
    """tier_table.compare over every gradient the truth holds; a gradient the truth holds and `hip` lacks is an error of its own
    (test_gpu_kkt checks the None pattern first)."""
    return T.compare(r, hip, t32, t64, keys=GRADS)
