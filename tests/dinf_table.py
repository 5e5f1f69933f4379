"""The cases of control['unbounded'], dual infeasibility detection under control['stop'] = 'each', and their truth (no GPU needed to
import this module).  tests/test_dinf_table.py checks them on the CPU, tests/test_gpu_dinf.py runs them.

The truth is `solve_certify`: ``oracle.solve_box_qp`` itself on a batch of one with ``infeas_table.Certificates`` as its per-check
callback, the dual certificate on behind the primal one.  In the SCALED problem, at a check of iteration k, against the snapshot
(x, Qs x) of the last check, valid iff it is the last check's and rho has not changed since:

    dx = x_k - x_prev;  dq = Qs x_k - Qs x_prev;  N = |dx|_inf
    e1 = |dq|_inf / N;  e2 = ps^T dx / N;  e3 = max_i([lbs_i finite] (-dx_i), [ubs_i finite] dx_i, 0) / N

and "dual infeasible" iff N > 0, e1 <= eps, e2 <= -eps and e3 <= eps: dx is a direction with Q dx = 0 and p^T dx < 0 inside the
recession cone of the box -- OSQP's certificate with differences taken check to check.  As dx is NOT tested (the x-update solves the
equality-constrained system, As x = bs holds at every iteration to rounding); `as_dx` records |As dx|_inf / N per check and
test_dinf_table.py bounds it at every detecting check.  Order in a check: optimal, primal infeasible, dual infeasible.  With the
dual threshold off it returns solve_detect's results, bit for bit.

A row is a row of ``each_table`` in which chosen problems are made unbounded without assuming what A looks like: a direction d with
m + 2 non-zero entries (drawn from the row's seed) is projected onto the null space of those columns of A; Q <- P Q P with
P = I - d d^T / d^T d, re-symmetrised; p loses its component along d and gets -f |p|_inf d / d^T d; the box is opened along d
(ub_i = +inf where d_i > 0, lb_i = -inf where d_i < 0).  ``gross``: f = 1; ``mild``: f = `f_mild`; ``open``: the same opened box with
Q and p left alone -- such a problem stays bounded and must come out optimal.  ``primal`` (the mixed row): infeas_table's `gross`
construction, b_0 moved out of reach.

Every row but the last sets check_solved = 30: between checks 10 iterations apart the binding terms fall by a factor of about 3, so no seed
could clear the threshold by a factor on both sides of a verdict; 30 apart they fall by about 10.  ``status`` and ``iters`` are what
the float32 AND the float64 truth give; the seeds were tried until, in both dtypes and with Qs x formed from the right-hand side,
every flagged verdict clears eps by MARGIN at the detecting check, misses by MARGIN at the valid check before it, and no problem
that is not flagged comes within MARGIN at any check (test_dinf_table.py recomputes all of it).  A condition on the inputs, not a
tolerance on the kernel.

A second condition on the inputs, for the comparison of a flagged problem's x: along the open null direction d nothing contracts,
x_d of iteration k + 1 is x_d of iteration k plus a step, so every iteration's rounding of x_d -- one unit roundoff u |x| at the very
least, u = 2^-24 in float32 -- stays in the iterate for good.  The bar of tests/test_gpu_each.py, 1e-5 |x|_inf, is 167 u: it can
only be asked of an iterate a float32 kernel reached in well under 167 iterations, whatever the order of its arithmetic.  The
float32 rows therefore hold only problems flagged by iteration FLAGGED_BY = 90, which leaves the bar room for about two roundings
per iteration (test_dinf_table.py checks it).  A draw of the split x4 family whose mild problem is flagged at iteration 150 was
tried first: on an MI355X its x stood 3.9e-5 from the float64 truth, against a bar of 2.4e-5 and 3.7e-6 for the float32 truth on
the CPU.  The float64 row carries no such limit.

The chunk_n20 row (the host-driven persistent schedule) checks at EVERY iteration: from one iteration to the next the binding terms
fall by a few per cent, so its verdicts hold a margin of 1.05, not 2 (`margin`; over the base row's seed and rho in {0.3, 1, 3} the
widest both dtypes give is 1.15), and it keeps the base row's seed, whose two long-running problems' counts test_each_table.py pins.
"""
import functools

import torch

from oracle import boxqp_oracle as O
import each_table as E
import infeas_table as IT

EPS = 1e-4           # control['eps_dual_inf'] (and eps_prim_inf) of every row: the defaults
MARGIN = 2.0
OPTIMAL, MAXITER, INFEASIBLE, UNBOUNDED = IT.OPTIMAL, IT.MAXITER, IT.INFEASIBLE, IT.UNBOUNDED
CHECK = 30
FLAGGED_BY = 90      # float32 rows: the last iteration at which a problem of the table is flagged (the module's docstring says why)

ROWS = {}


def make_row(name, base, tier, gross, mild, open_, status=None, iters=None, f_mild=0.1, primal=(), check=CHECK, margin=MARGIN,
             rho_b=None, **kw):
    """base: the each_table row it builds on (kw: what differs); tier: (loop_kind, workgroups per QP) as test_gpu_each.py asserts;
    check: the row's check_solved; margin: the factor its verdicts hold; rho_b: one given rho per problem"""
    row = dict(E.ROWS[base], **kw)
    row.update(name=name, base=base, tier=tier, gross=list(gross), mild=list(mild), open=list(open_), primal=list(primal),
               status=status, iters=iters, f_mild=f_mild, check=check, margin=margin, rho_b=rho_b, infeasible_last=False, never=[],
               adapts=None)
    return row


def _row(name, *a, **kw):
    ROWS[name] = make_row(name, *a, **kw)


def direction(row, i, A):
    """-> d (n,): m + 2 non-zero entries on indices drawn from the row's seed, projected onto the null space of those columns of A_i"""
    n, m = row["n"], row["m"]
    g = torch.Generator().manual_seed(7919 * row["seed"] + i)
    idx = torch.randperm(n, generator=g)[:m + 2]
    v = torch.randn(m + 2, generator=g, dtype=torch.float64)
    if m > 0:
        As = A[i][:, idx]
        v = v - As.T @ torch.linalg.solve(As @ As.T, As @ v)
    d = torch.zeros(n, dtype=torch.float64)
    d[idx] = v
    return d


def inputs(row, dtype=torch.float64):
    """-> Q, p, A, b, lb, ub: each_table's inputs of the row with the `gross` / `mild` problems made unbounded, the box of the `open`
    ones opened the same way and b_0 of the `primal` ones moved out of reach"""
    Q, p, A, b, lb, ub = E.inputs(row, torch.float64)
    inf = float("inf")
    for idx, f in ((row["gross"], 1.0), (row["mild"], row["f_mild"]), (row["open"], None)):
        for i in idx:
            d = direction(row, i, A)
            dd = float(d @ d)
            if f is not None:
                P = torch.eye(row["n"], dtype=torch.float64) - torch.outer(d, d) / dd
                Qi = P @ Q[i] @ P
                Q[i] = (Qi + Qi.T) / 2
                pi = p[i, :, 0]
                pi = pi - (pi @ d) * d / dd
                p[i, :, 0] = pi - f * float(pi.abs().max()) * d / dd
            ub[i, :, 0] = torch.where(d > 0, torch.full_like(d, inf), ub[i, :, 0])
            lb[i, :, 0] = torch.where(d < 0, torch.full_like(d, -inf), lb[i, :, 0])
    for i in row["primal"]:
        IT.out_of_reach(A, b, lb, ub, i, 1.0)
    cast = lambda t: None if t is None else t.to(dtype).contiguous()
    return tuple(cast(t) for t in (Q, p, A, b, lb, ub))


def control(row, problem=None, **extra):
    """the oracle's control of the row; problem: of that problem solved alone (rows with one rho per problem, `rho_b`).  check_solved
    is set on the dict: the factory, like the reference's, files its argument under a key the solver never reads"""
    if problem is not None and row.get("rho_b") is not None:
        extra = dict(extra, rho=float(row["rho_b"][problem]))
    ctl = O.make_control(**dict(row["control"], **extra))
    ctl["check_solved"] = row["check"]
    return ctl


def solve_certify(Q, p, A, b, lb, ub, control, eps_prim_inf=None, eps_dual_inf=None, bounds=None, qx_from_rhs=False):
    """``infeas_table.solve_detect`` with the dual certificate behind the primal one at every check (either threshold None: that
    certificate is off).  -> solve_detect's dict (status 3: dual infeasible) plus "dchecks" and "as_dx" (``infeas_table.Certificates``)."""
    cert = IT.Certificates(eps_prim_inf, eps_dual_inf, qx_from_rhs)
    sol = IT.solve_with(cert, Q, p, A, b, lb, ub, control, bounds)
    sol.update(dchecks=cert.dchecks, as_dx=cert.as_dx)
    return sol


def solve_row(row, dtype, primal=None, dual=True, qx_from_rhs=False):
    """-> every problem of the row solved by solve_certify as a batch of one (the bound flags of the whole batch: both finite).
    primal: the primal certificate too (None: iff the row holds `primal` problems -- the mixed row runs with both keys)"""
    primal = bool(row["primal"]) if primal is None else primal
    qp = inputs(row, dtype)
    return [solve_certify(*E.alone(qp, i), control(row, problem=i), eps_prim_inf=EPS if primal else None,
                          eps_dual_inf=EPS if dual else None, qx_from_rhs=qx_from_rhs, **E.ALONE) for i in range(row["B"])]


@functools.lru_cache(maxsize=None)
def truth(name, dtype, dual=True, qx_from_rhs=False):
    return solve_row(ROWS[name], dtype, dual=dual, qx_from_rhs=qx_from_rhs)


def dual_miss(e1, e2, e3, eps=EPS):
    """by what factor the dual rule misses at a check (< 1: it holds)"""
    return max(e1 / eps, eps / max(-e2, 1e-300), e3 / eps)


def margins(sol, eps=EPS):
    """How far the dual rule is from its verdict over the checks of one solve -> (clear, miss_before, nearest): clear: 1 / miss at the
    detecting check (None: not flagged dual infeasible); miss_before: the miss at the valid check before it (None: there is
    none); nearest: over the checks that did not flag, the smallest miss (inf: never a valid snapshot with N > 0)."""
    miss = lambda e1, e2, e3: dual_miss(e1, e2, e3, eps)
    last, miss_before, nearest = IT.margins_of(sol["dchecks"], sol["status"] == UNBOUNDED, miss, 5)
    clear = None if last is None else 1.0 / max(miss(*last), 1e-300)
    return clear, miss_before, nearest


# (loop_kind, workgroups per problem) as last_forward_status names them: 2 the small loop, 1 the split loop, 0 the one-workgroup loop
SMALL, SPLIT2, SPLIT4, ONE = IT.SMALL, IT.SPLIT2, IT.SPLIT4, IT.ONE
_RHO1 = IT._RHO1      # the event recipe with a given rho 100 times too small: the event (iteration 90 with a check every 30) fires for
                      # every problem that still runs -- the unbounded ones are detected BEHIND it

_EVENT30 = dict(_RHO1, adaptive_rho_iter=30, rho_min=0.5)
# (with a check every 30 the certificate of these fast-converging problems forms at iteration 60, in front of the recipe's own event
#  at 90: the event is moved to iteration 30, so that the check at 30 only refreshes the snapshot and the problems are flagged at the
#  first valid check behind it.  An unbounded problem's primal residual vanishes while its dual one does not, so the event drives its
#  rho down to rho_min, and x_d = (...) / rho along the null direction takes the condition number of Qs + rho I with it: at
#  rho_min = 0.01 the float32 and the float64 truth of a flagged x already stand 2e-3 |x|_inf apart.  0.5 -- half the given rho --
#  keeps the solve as well conditioned as in front of the event; the event at iteration 60 then leaves rho where it is)

_row("small_n50", "small_n50_event", SMALL, gross=[0], mild=[1], open_=[3], control=E.PLAIN, q_scale=1., p_decades=5., seed=4,
     status=[3, 3, 0, 0, 0, 0, 0, 0], iters=[60, 90, 60, 60, 30, 30, 0, 0])
_row("split_n130", "split_n130", SPLIT2, gross=[1], mild=[0], open_=[3], seed=3,
     status=[3, 3, 0, 0, 0, 0, 0, 0], iters=[60, 90, 90, 60, 30, 30, 0, 0])
_row("split_n449", "split_n449", SPLIT4, gross=[1], mild=[0], open_=[3], seed=1,
     status=[3, 3, 0, 0, 0, 0, 0, 0], iters=[60, 90, 90, 60, 30, 30, 30, 0])
_row("split_n130_event", "split_n130_event", SPLIT2, gross=[0], mild=[2], open_=[1], control=_EVENT30, seed=1,
     status=[3, 0, 3, 0, 0, 0, 0, 0], iters=[60, 30, 60, 30, 0, 0, 0, 0])
# (17 equality rows: with f = 0.1 the mild problems of this family are flagged at iteration 120 - 150, see FLAGGED_BY; f = 0.3)
_row("lu_n130_m17", "lu_n130_m17", ONE, gross=[1], mild=[0], open_=[2], f_mild=0.3, seed=3,
     status=[3, 3, 0, 0, 0, 0], iters=[90, 90, 60, 30, 30, 0])
_row("f64_n70_m3", "f64_n70_m3", ONE, gross=[1], mild=[2], open_=[3], seed=3,
     status=[0, 3, 3, 0, 0, 0, 0, 0], iters=[30, 90, 150, 60, 30, 30, 0, 0])
# a batch of two: one unbounded problem, flagged behind its event, next to a feasible one with the opened box
_row("big_n1030", "big_n1030", ONE, gross=[0], mild=[], open_=[1], control=dict(_EVENT30, max_iters=400), seed=1,
     status=[3, 0], iters=[60, 0])
# both keys: a primal infeasible problem (infeas_table's `gross`) and unbounded ones in one batch, statuses 2 and 3
_row("mixed_n130", "split_n130", SPLIT2, gross=[1], mild=[0], open_=[3], primal=[2], seed=3,
     status=[3, 3, 2, 0, 0, 0, 0, 0], iters=[60, 90, 60, 60, 30, 30, 0, 0])
# The host-driven persistent schedule with a check at EVERY iteration (see the module's docstring for its margin).  The base row's
# rho = 0.003 keeps two problems running through the chunk boundaries; the unbounded ones get a rho of their own, 0.3, and are flagged
# early, as infeas_table's row of this family does it.  Problem 5 is the base row's, without its unreachable b.
_row("chunk_n20", "chunk_n20", ONE, gross=[2], mild=[3], open_=[4], f_mild=0.3, seed=4, check=1, margin=1.05,
     rho_b=[0.003, 0.003, 0.3, 0.3, 0.003, 0.003], status=[1, 0, 3, 3, 0, 0], iters=[1199, 600, 27, 25, 0, 0])
