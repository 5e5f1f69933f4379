"""The fixed-point backward (lqp_boxqp_backward_fp), as data (no GPU needed to import this module).

The backward is a function of (cot, x, u, lams, nus, Q, A, lb, ub, rho) alone, so a row does not solve anything: `point` builds a
synthetic fixed point in float64 whose FREE SET HAS THE SIZE THE ROW ASKS FOR and rounds it ONCE to the row's dtype; the GPU call, the
float32 oracle (the budget) and the float64 oracle (the truth, on the float32 values converted exactly) receive the same numbers.
What selects the code of the Cholesky form is the block count of the free set, Kb = ceil(|F| / 64), per problem -- not n: the rows
put |F| on 64 k and 64 k + 1, mix block counts inside one launch, make it tiny under a large n, equal to n, and 0.
tests/test_gpu_fp.py runs every row on the GPU against oracle.boxqp_oracle.solve_box_qp_grad with tier_table.compare, all six
gradients (float32 rows |hip - t64| <= R |t32 - t64| + F scale, float64 rows 1e-9 scale), and checks which form ran;
tests/test_fp_table.py checks, without a GPU, the free sets, the budgets, the oracle against a hand-written reduced solve, the
coverage of the rows and that the comparator sees errors.

Row fields:
  name, n, m, dtype ("f32" | "f64"), B (int, or an expression of `cus`; a list `nf` sets it)
  nf       size of the free set: an int, a list with one value per problem, or "n"
  entry    "chol":     SB._fp_backward(..., linsolve=2), one call -- what the module calls behind the symmetric forward
           "chol_pre": SB._fp_backward_prepare(..., linsolve=2, prefactor=True), then SB._fp_backward_run: phases 1 and 2
           "lu":       L.torch_solve_box_qp_grad (linsolve 1: the reduced system's pivoted LU with its refinement step)
           "lu_pre":   the same in two phases (prefactor=True)
  rho      None | a float | "tensor" (a (B,1,1) tensor, another value per problem): dlb / dub = kkt / (rho u) alone read it
  q        "sym" | "nonsym" | "indef" (symmetric, one eigenvalue moved to -0.5 along free variables: Q_FF is not positive definite,
           the reduced system is regular)
  form     the form that must have run, by launch classes of _lib.profile(): FORMS[form], one count per PROF_CLASSES
  env      LQP_* overrides; flip / same / R / F / why as in tests/tier_table.py
  want     True: the row also calls with subsets of `want`; the outputs still asked for must keep their bits
"""
import torch

import tier_table as T

GRADS = ("dQ", "dp", "dA", "db", "dlb", "dub")
# (bwd_build counts k_bwd_build_chol / k_bwd_build_reduced / k_bwd_build, k_bwd_gather_rhs and k_bwd_residual alike)
PROF_CLASSES = ("bwd_build", "bwd_cholesky", "lu_factor", "pack", "packed_solve", "bwd_epilogue")
FORMS = {
    "chol": (1, 1, 0, 0, 0, 1),          # build, k_bwd_chol_solve (factor and solves), epilogue
    "chol_pre": (1, 2, 0, 0, 0, 1),      # phase 1: build, factor | phase 2: solves (the kernel gathers the cotangent itself), epilogue
    "lu": (2, 0, 1, 1, 2, 1),            # build, LU, pack, solve | residual, correction solve | epilogue
    "lu_pre": (3, 0, 1, 1, 2, 1),        # phase 1: build, LU, pack | phase 2: gather, solve, residual, correction solve, epilogue
    "lu_once": (1, 0, 1, 1, 1, 1),       # no refinement step: LQP_BWD_REFINE=0, and the full system of LQP_BWD_FULL=1
    "fallback": (3, 1, 1, 1, 2, 2),      # the Cholesky attempt reports "not positive definite", the call repeats itself on the LU form
}
ENTRIES = ("chol", "chol_pre", "lu", "lu_pre")
RHOS = ("none", "float", "tensor")


def row(name, n, m, nf, B=3, dtype="f32", entry="chol", env=None, q="sym", rho=None, form=None, R=T.R_DEFAULT, F=T.F_DEFAULT,
        flip=None, same=False, want=False, why=None):
    env = dict(env or {})
    if isinstance(nf, list):
        B = len(nf)
    return dict(name=name, n=n, m=m, nf=nf, B=B, dtype=dtype, entry=entry, env=env, q=q, rho=rho, form=form or entry, R=R, F=F,
                flip=(dict(flip) if flip is not None else ({} if env else None)), same=same, want=want, why=why)


ROWS = [
    # ---------------- Cholesky form: block counts of the free set ----------------
    row("chol_nf1_n130", 130, 0, 1, why="one free variable: one block, 63 rows of identity padding"),
    row("chol_nf63_n130", 130, 1, 63),
    row("chol_nf64_n150", 150, 2, 64, want=True, why="a full block, no padding"),
    row("chol_nf65_n150", 150, 1, 65, rho=0.7, why="two blocks, one entry in the second"),
    row("chol_nf128_n200", 200, 0, 128),
    row("chol_nf129_n200", 200, 1, 129, rho="tensor"),
    row("chol_nf448_449_n512", 512, 1, [448, 449], why="Kmax = 8, la_maxk = 7: the look-ahead and wg_chol_factor in one launch"),
    row("chol_nf448_449_n576", 576, 2, [448, 449], why="Kmax = 9, la_maxk stays 7"),
    row("chol_nf512_513_n576", 576, 1, [512, 513], why="wg_chol_factor | wg_chol_factor_big in one launch"),
    row("chol_nfn_n64", 64, 1, "n", why="every variable free, the lb == ub ones at their bound with u = 0"),
    row("chol_nfn_n449", 449, 1, "n", B=2),
    row("chol_nfn_n1024", 1024, 0, "n", B=2, why="16 blocks, Kb = Kmax"),
    row("chol_nf65_n1024", 1024, 1, 65, B=2, why="two blocks under the largest Ls stride"),
    row("chol_nf1_n1024", 1024, 0, 1, B=2, why="one free variable under the largest LDS layout"),
    row("chol_mixed_n576", 576, 0, [1, 64, 65, 448, 449, 513], rho="tensor",
        why="every factor routine and six block counts in one launch; Ls strided by sym_blocks(9), indexed by Kb"),
    row("chol_mixed_m2_n576", 576, 2, [30, 64, 65, 448, 449, 513], why="the same with equality rows (nf >= m + 8)"),
    # ---------------- equality rows (Cholesky form) ----------------
    row("chol_m3_nf200_n330", 330, 3, 200, why="m = 3: the first four-right-hand-side instance"),
    row("chol_m16_nf100_n200", 200, 16, 100, rho=0.7),
    row("chol_m16_nf600_n1024", 1024, 16, 600, B=2, why="m = 16 at the largest LDS layout"),
    # ---------------- the empty free set: Kb = 0 skips factor and solves; dv = 0, dnu = 0, dlb / dub from kkt = -g ----------------
    row("chol_nf0_m0_n130", 130, 0, 0, rho=0.7),
    row("chol_nf0_m1_n130", 130, 1, 0, rho="tensor"),
    row("chol_nf0_among_n200", 200, 2, [0, 10, 0, 70], why="empty free sets among others in one launch"),
    row("lu_nf0_m1_n130", 130, 1, 0, entry="lu"),
    row("lu_nf0_m0_n130", 130, 0, 0, entry="lu", rho=0.7,
        why="Nvec[b] = 0: the LU kernels, the pack and both solves run no step at all (read, not tried: every loop bound is the size)"),
    row("lu_pre_nf0_m1_n130", 130, 1, 0, entry="lu_pre", dtype="f64", rho=0.7),
    # ---------------- prefactored calls: the same bits as the one-call form on the same point ----------------
    row("chol_pre_nf65_n150", 150, 1, 65, entry="chol_pre", want=True),
    row("chol_pre_nf449_n512", 512, 2, 449, B=2, entry="chol_pre", rho="tensor"),
    row("chol_pre_nf513_n576", 576, 1, 513, B=2, entry="chol_pre"),
    row("lu_pre_n150_f64", 150, 2, 80, entry="lu_pre", dtype="f64"),
    # ---------------- LU forms: Nvec[b] = |F| + m per problem ----------------
    row("lu_nf1_n130_f64", 130, 0, 1, entry="lu", dtype="f64"),
    row("lu_nf64_n150_f64", 150, 1, 64, entry="lu", dtype="f64", rho="tensor"),
    row("lu_nf65_n150_f64", 150, 2, 65, entry="lu", dtype="f64", rho=0.7),
    row("lu_nf257_n300_f64", 300, 3, [257, 30, 256], entry="lu", dtype="f64"),
    row("lu_nf100_n200", 200, 2, 100, entry="lu", rho=0.7),
    row("lu_refine0_nf100_n200", 200, 2, 100, entry="lu", env={"LQP_BWD_REFINE": "0"}, form="lu_once"),
    row("lu_full_nf100_n200", 200, 1, 100, entry="lu", env={"LQP_BWD_FULL": "1"}, form="lu_once", rho="tensor"),
    row("lu_full_nf80_n150_f64", 150, 2, [80, 0, 149], entry="lu", dtype="f64", env={"LQP_BWD_FULL": "1"}, form="lu_once"),
    row("planner_m17_n200", 200, 17, 120, form="lu", why="m > 16: the planner itself leaves the Cholesky form"),
    row("planner_n1025_m0", 1025, 0, 300, B=2, form="lu", why="17 blocks: the planner itself leaves the Cholesky form"),
    row("lu_nonsym_nf150_n300", 300, 1, 150, entry="lu", q="nonsym"),
    row("lu_split2off_nf100_n200", 200, 2, 100, entry="lu", env={"LQP_SPLIT2": "0"}, same=True,
        why="the second workgroup per problem takes whole rows of the build, pack and residual kernels: the same bits (measured)"),
    row("lu_n1100_f64", 1100, 1, 500, B=1, entry="lu", dtype="f64"),
    # ---------------- Q_FF not positive definite: the Cholesky attempt gives up, the call repeats on the LU form ----------------
    row("fallback_indef_n200", 200, 1, 120, q="indef", form="fallback"),
    # ---------------- knobs ----------------
    row("chol_f16off_nf200_n330", 330, 1, 200, env={"LQP_BWD_F16": "0"}, why="Kb = 4: float32 tile products in the look-ahead"),
    row("chol_spdf16off_nf200_n330", 330, 2, 200, env={"LQP_SPD_F16": "0"}, why="Kb = 4: the same switch by its other name"),
    row("chol_equil0_nf200_n330", 330, 1, 200, env={"LQP_BWD_EQUIL": "0"}, why="Kb = 4: the float16 operands without the equilibration"),
    row("chol_la0_nf200_n330", 330, 2, 200, env={"LQP_BWD_LOOKAHEAD": "0"}, why="Kb = 4 on wg_chol_factor: float32 products"),
    row("chol0_nf100_n200", 200, 2, 100, env={"LQP_BWD_CHOL": "0"}, form="lu"),
    row("chol_early0_nf100_n200", 200, 1, 100, env={"LQP_BWD_EARLY": "0"}, same=True,
        why="which launch stores the info words for the host does not touch the arithmetic (measured: same bits)"),
    row("chol_slabs1_nf200_n330", 330, 2, 200, env={"LQP_EPI_SLABS": "1"}, same=True,
        why="the epilogue computes every row of dQ, dlb and dub whole, whichever slab it falls into (measured: same bits)"),
    # ---------------- batch sizes ----------------
    row("chol_nf70_n130_cus3", 130, 1, 70, B="cus + 3", why="small_batch_split gives one slab"),
]

ROW_BY_NAME = {r["name"]: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS), "duplicate row names"

# the knobs of docs/KNOBS.md the backward's plan reads (plan_backward, enqueue_*): every LQP_BWD_* and these three
BACKWARD_KNOBS_EXTRA = ("LQP_EPI_SLABS", "LQP_SPLIT2", "LQP_SPD_F16")
# ... and those among them the fixed-point backward does not read, each with its reason (none: it reads them all)
NOT_READ = {}

# the rows in which dv = 0 and dnu = 0 exactly in both precisions (every free set of the row empty): the float32 budget of
# dQ, dp, dA, db is zero there, and so must the GPU's error be
ZERO_BUDGET = ("chol_nf0_m0_n130", "chol_nf0_m1_n130", "lu_nf0_m1_n130", "lu_nf0_m0_n130", "lu_pre_nf0_m1_n130")

# thresholds of plan_backward / k_bwd_chol_solve: (key, lower side, upper side); "Kb" = ceil(|F| / 64) of a problem on the Cholesky form
THRESHOLDS = {
    "Kb 1 | 2": ("Kb", 1, 2),
    "Kb 7 | 8 (look-ahead | wg_chol_factor)": ("Kb", 7, 8),
    "Kb 8 | 9 (wg_chol_factor | wg_chol_factor_big)": ("Kb", 8, 9),
    "n 1024 | 1025 (Cholesky form | LU)": ("n", 1024, 1025),
    "m 2 | 3 (two | four right-hand sides per round)": ("m_chol", 2, 3),
    "m 16 | 17 (Cholesky form | LU)": ("m", 16, 17),
    "nf 0 | 1": ("nf", 0, 1),
}


def ran_chol(r):
    return r["form"] in ("chol", "chol_pre")


def nf_of(r, i):
    """Size of the free set of problem i."""
    nf = r["nf"]
    if nf == "n":
        return r["n"]
    return nf[i] if isinstance(nf, list) else nf


def nf_values(r):
    nf = r["nf"]
    return {r["n"]} if nf == "n" else set(nf) if isinstance(nf, list) else {nf}


def threshold_values(key, r):
    """The row's values for a threshold key (a row with a list `nf` holds several): empty when the row does not bear on it."""
    if key == "Kb":
        return {T.ks(v) for v in nf_values(r)} if ran_chol(r) else set()
    if key == "m_chol":
        return {r["m"]} if ran_chol(r) else set()
    if key == "nf":
        return nf_values(r)
    return {r[key]} if r["entry"] in ("chol", "chol_pre") else set()   # (n, m: what the planner decides on when asked for the Cholesky form)


def dtype_of(r):
    return torch.float32 if r["dtype"] == "f32" else torch.float64


def rho_kind(r):
    return "none" if r["rho"] is None else "tensor" if r["rho"] == "tensor" else "float"


def none_pattern(r):
    """Which of GRADS the reference returns as None for this row."""
    return dict(dQ=False, dp=False, dA=r["m"] == 0, db=r["m"] == 0, dlb=False, dub=False)


def _point(r, i, qcache):
    """Problem i of the row, float64 values that the row's dtype holds exactly where it matters:
    (cot, x, u, lams, nus, Q, A, lb, ub, rho) with Q / A / bounds of tier_table._problem (some lb = -inf, some ub = +inf, a few
    lb == ub; bounds rounded to the row's dtype here, so that `x = bound` survives the rounding) and exactly nf_of(r, i) free
    variables.  A variable is made ACTIVE only on a side where its bound is finite: x = that bound, u = -k/64 (lower) or +k/64
    (upper), k in 1..64 -- exact in float32, so x + u compares with the bound in the same way in float32 and float64 --, and k'/64
    in the matching half of lams.  FREE variables have u = 0 and lam = 0, interior except up to three per problem that sit exactly on
    a finite bound (x + u == ub is free under the reference's strict comparison).  The variable with the largest index is free whenever
    nf > 0 (the last, partial 64-block of Q bears on dv); lb == ub variables are active while the row's nf leaves room for that, free
    at their bound otherwise.  tier_table._problem leaves about one variable in 77 without any finite bound: where the row's nf
    needs more active variables than there are bounded ones, those variables receive a finite lower bound here (rows with nf < n / 77)."""
    n, m = r["n"], r["m"]
    nf = nf_of(r, i)
    assert 0 <= nf <= n and (m == 0 or nf == 0 or nf >= m + 8), (r["name"], i, nf)
    dt = dtype_of(r)
    Q, _, A, _, lb, ub = T._problem(r, i, qcache)
    g = torch.Generator().manual_seed(T.seed_of(r) * 104729 + i)
    rnd = lambda: torch.rand(n, 1, generator=g, dtype=torch.float64)
    frac, side, newlb = rnd(), rnd(), -(1.0 + rnd())
    ku = torch.randint(1, 65, (n, 1), generator=g).double() / 64
    kl = torch.randint(1, 65, (n, 1), generator=g).double() / 64
    perm = torch.randperm(n - 1, generator=g).tolist()
    nus = torch.randn(m, 1, generator=g, dtype=torch.float64) if m else None
    cot = torch.randn(n, 1, generator=g, dtype=torch.float64)
    # ---- who is active ----
    n_act = n - nf
    flb, fub = torch.isfinite(lb).squeeze(1), torch.isfinite(ub).squeeze(1)
    fixed = (flb & fub & (lb == ub).squeeze(1)).tolist()
    bounded = (flb | fub).tolist()
    order = [j for j in perm if fixed[j]] + [j for j in perm if bounded[j] and not fixed[j]]
    if len(order) + (1 if nf == 0 and bounded[n - 1] else 0) < n_act:
        lb = torch.where((~(flb | fub)).unsqueeze(1), newlb, lb)
        flb = torch.isfinite(lb).squeeze(1)
        order = order + [j for j in perm if not bounded[j]]
        bounded = [True] * n
    if nf == 0:
        order = order + [n - 1]
    assert len(order) >= n_act and bounded[n - 1] >= (nf == 0), (r["name"], i, "not enough variables with a finite bound")
    lb, ub = lb.to(dt).double(), ub.to(dt).double()
    act = torch.zeros(n, dtype=torch.bool)
    act[order[:n_act]] = True
    free = ~act
    # ---- the point ----
    lo = torch.where(flb.unsqueeze(1), lb, torch.full_like(lb, -3.0))
    hi = torch.where(fub.unsqueeze(1), ub, torch.full_like(ub, 3.0))
    x = lo + (hi - lo) * (0.1 + 0.8 * frac)
    u, lam_lo, lam_hi = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    at_ub = act & fub & ((side.squeeze(1) < 0.5) | ~flb)
    at_lb = act & ~at_ub
    assert bool(flb[at_lb].all()) and bool(fub[at_ub].all())
    a_ub, a_lb = at_ub.unsqueeze(1), at_lb.unsqueeze(1)
    x = torch.where(a_ub, ub, torch.where(a_lb, lb, x))
    u = torch.where(a_ub, ku, torch.where(a_lb, -ku, u))
    lam_hi = torch.where(a_ub, kl, lam_hi)
    lam_lo = torch.where(a_lb, kl, lam_lo)
    # free variables exactly on a bound: every free lb == ub variable, and up to three others (never the last variable)
    ties = [j for j in range(n) if free[j] and fixed[j]]
    ties += [j for j in perm if free[j] and bounded[j] and not fixed[j]][:min(3, max(nf - 1, 0))]
    for c, j in enumerate(ties):
        x[j] = ub[j] if (fub[j] and (c % 2 == 0 or not flb[j])) else lb[j]
    if r["q"] == "indef":
        v = torch.randn(n, 1, generator=g, dtype=torch.float64) * free.unsqueeze(1)
        v = v / v.norm()
        Q = Q - (float(v.T @ Q @ v) + 0.5) * (v @ v.T)
    rho = None if r["rho"] is None else torch.full((1, 1), 0.5 + 0.25 * (i % 7) if r["rho"] == "tensor" else float(r["rho"]), dtype=torch.float64)
    return cot, x, u, torch.cat((lam_lo, lam_hi), 0), nus, Q, A, lb, ub, rho


def point(r, B, idx=None):
    """(cot, x, u, lams, nus, Q, A, lb, ub, rho) of the batch -- or of the problems `idx` of it -- rounded once to the row's dtype.
    rho: None, a float, or a (B,1,1) tensor."""
    dt = dtype_of(r)
    qcache = {}
    parts = [_point(r, i, qcache) for i in (range(B) if idx is None else idx)]
    out = [None if parts[0][k] is None else torch.stack([pt[k] for pt in parts]).to(dt) for k in range(10)]
    if r["rho"] != "tensor" and out[9] is not None:
        out[9] = float(r["rho"])
    return tuple(out)


def free_set(pt, dtype):
    """The reference's mask (:360-365) of the point evaluated in `dtype`: True where the variable is free."""
    x, u, lb, ub = (pt[k].to(dtype) for k in (1, 2, 7, 8))
    w = x + u
    return ~((w > ub) | (w < lb)).squeeze(2)


def oracle(pt, dtype, hook=None):
    """The CPU oracle's fixed-point backward of the point `pt` in `dtype` -> {name: tensor or None}.  `hook` (tests of the
    comparator) maps the converted arguments to wrong ones."""
    from oracle import boxqp_oracle as O
    args = [t.to(dtype) if torch.is_tensor(t) else t for t in pt]
    if hook is not None:
        args = hook(args)
    return dict(zip(GRADS, O.solve_box_qp_grad(*args)[:6]))


def compare(r, hip, t32, t64):
    """tier_table.compare over every gradient the truth holds; a gradient the truth holds and `hip` lacks is an error of its own
    (test_gpu_fp checks the None pattern first)."""
    return T.compare(r, hip, t32, t64, keys=GRADS)
