"""The cases of control['infeasible'], primal infeasibility detection under control['stop'] = 'each', and their truth (no GPU
needed to import this module).  tests/test_infeas_table.py checks them on the CPU, tests/test_gpu_infeas.py runs them.

The truth is `solve_detect`: ``oracle.solve_box_qp`` itself, the one loop the reference-made goldens pin, on a batch of one with
`Certificates` as its per-check callback (``at_check``).  `Certificates` holds the primal rule below and the dual one that
tests/dinf_table.py describes.  In the SCALED problem, after the element-wise update of iteration k:

    y = rho u_k;  g = Qs x_k + rho (z_k - z_{k-1});  nu = nu_k

against the snapshot (y, g, nu) of the last check, which is valid iff rho has not changed since:

    dy, dg, dnu;  N = |dy|_inf;  c1 = |dg|_inf / N;  c2 = (sum_i [ubs_i max(dy_i, 0) + lbs_i min(dy_i, 0)] + bs^T dnu) / N

(a term of an infinite bound counts 0 while |dy_i| <= eps N, else c2 = +inf) and "primal infeasible" iff N > 0, c1 <= eps and
c2 <= -eps.  Optimal comes first; a flagged problem stops with the iterate of that check.  With detection off the callback changes
no bit of the solve (test_infeas_table.py).

A row is a row of ``each_table`` (its inputs, its control) in which chosen problems are made infeasible without assuming what A
looks like: with lo / hi the smallest / largest value of A_0 x over the box, b_0 = hi + f (hi - lo) -- ``gross``: f = 1,
``mild``: f = 0.02.  One row per kernel family at the smallest shape that reaches it (the shapes of each_table).  ``status`` and
``iters`` are what the float32 AND the float64 truth give; the seeds were tried until, in both dtypes, c1 and -c2 clear
eps_prim_inf by a factor MARGIN at the detecting check of every flagged problem, the rule misses by that factor at the valid
check before, and no feasible problem comes within that factor of being flagged at any check (test_infeas_table.py recomputes
all of it).  The factor is a condition on the inputs, not a tolerance on the kernel: a verdict that hangs on rounding would make
the GPU comparison a coin toss.
"""
import functools

import torch

from oracle import boxqp_oracle as O
import each_table as E

EPS = 1e-4           # control['eps_prim_inf'] of every row (the default)
MARGIN = 4.0
OPTIMAL, MAXITER, INFEASIBLE, UNBOUNDED = 0, 1, 2, 3      # (3: the dual certificate, tests/dinf_table.py)

ROWS = {}


def _row(name, base, tier, gross, mild, status, iters, f_mild=0.02, margin=MARGIN, rho_b=None, **kw):
    """base: the each_table row it builds on (kw: what differs); tier: (loop_kind, workgroups per QP) as test_gpu_each.py asserts;
    f_mild: the f of the `mild` problems where 0.02 gives no row that holds the margin; rho_b: one given rho per problem"""
    row = dict(E.ROWS[base], **kw)
    row.update(name=name, tier=tier, gross=gross, mild=mild, status=status, iters=iters, f_mild=f_mild, margin=margin, rho_b=rho_b,
               infeasible_last=False, never=[], adapts=None)
    ROWS[name] = row


def out_of_reach(A, b, lb, ub, i, f):
    """moves b_0 of problem i out of reach, in place: b_0 = hi + f (hi - lo), lo / hi the smallest / largest A_0 x over the box"""
    a0 = A[i, 0]
    hi = float((a0 * torch.where(a0 > 0, ub[i, :, 0], lb[i, :, 0])).sum())
    lo = float((a0 * torch.where(a0 > 0, lb[i, :, 0], ub[i, :, 0])).sum())
    b[i, 0, 0] = hi + f * (hi - lo)


def inputs(row, dtype=torch.float64):
    """-> Q, p, A, b, lb, ub: each_table's inputs of the row with b_0 of the `gross` / `mild` problems moved out of reach"""
    Q, p, A, b, lb, ub = E.inputs(row, torch.float64)
    for idx, f in ((row["gross"], 1.0), (row["mild"], row.get("f_mild", 0.02))):
        for i in idx:
            out_of_reach(A, b, lb, ub, i, f)
    cast = lambda t: None if t is None else t.to(dtype).contiguous()
    return tuple(cast(t) for t in (Q, p, A, b, lb, ub))


def control(row, problem=None, **extra):
    """the oracle's control of the row; problem: of that problem solved alone (rows with one rho per problem, `rho_b`)"""
    if problem is not None and row.get("rho_b") is not None:
        extra = dict(extra, rho=float(row["rho_b"][problem]))
    return O.make_control(**dict(row["control"], **extra))


class Certificates:
    """The primal and the dual infeasibility certificate as the ``at_check`` callback of ``oracle.solve_box_qp`` on a batch of ONE
    (a threshold of None: that certificate is off; both None: the callback looks at nothing).  It owns the snapshot
    (y, g, nu, rho, iteration, x, Qs x) of the last check it was called at, which is valid iff that was the check before this one and
    rho has not changed since, and the records: `checks`, per check (iteration, c1, c2, N, valid) of the primal rule; `dchecks`,
    per check (iteration, e1, e2, e3, N, valid) of the dual rule (tests/dinf_table.py), and `as_dx`: |As dx|_inf / N of the same
    checks -- the terms None where there was no valid snapshot or N == 0.  Order in a check: primal infeasible (-> 2), dual
    infeasible (-> 3).  qx_from_rhs: Qs x is w - rho x - As^T nu, as a kernel that does not touch Q forms it, not the product (the
    rows' verdicts must not care)."""

    def __init__(self, eps_prim_inf=None, eps_dual_inf=None, qx_from_rhs=False):
        self.eps_prim_inf, self.eps_dual_inf, self.qx_from_rhs = eps_prim_inf, eps_dual_inf, qx_from_rhs
        self.snap = None
        self.checks, self.dchecks, self.as_dx = [], [], []

    def __call__(self, it, st):
        assert st.B == 1
        if self.eps_prim_inf is None and self.eps_dual_inf is None:
            return 0
        n, m, x, rho = st.n, st.m, st.x, st.rho
        rho_now = float(torch.as_tensor(rho).reshape(-1)[0])
        nu = st.xv[:, n:, :] if m > 0 else torch.zeros(1, 0, 1, dtype=x.dtype)
        qx = st.qx
        if self.qx_from_rhs:
            qx = st.rhs[:, :n, :] - rho * x - (torch.matmul(st.As.transpose(1, 2), nu) if m > 0 else 0)
        y, g = rho * st.u, qx + st.s
        prev = self.snap
        valid = prev is not None and prev[3] == rho_now and prev[4] == it - st.check_solved
        self.snap = (y.clone(), g.clone(), nu.clone(), rho_now, it, x.clone(), qx.clone())
        if self.eps_prim_inf is not None and self._primal(it, st, valid, prev, y, g, nu):
            return INFEASIBLE
        if self.eps_dual_inf is not None and self._dual(it, st, valid, prev, x, qx):
            return UNBOUNDED
        return 0

    @staticmethod
    def _whole(t, like):
        return torch.broadcast_to(torch.as_tensor(t, dtype=like.dtype), like.shape)

    def _primal(self, it, st, valid, prev, y, g, nu):
        eps = self.eps_prim_inf
        c1 = c2 = N = None
        if valid:
            dy, dg, dnu = y - prev[0], g - prev[1], nu - prev[2]
            N = float(dy.abs().max())
            if N > 0:
                c1 = float(dg.abs().max()) / N
                bnd = torch.where(dy > 0, self._whole(st.ubs, dy), self._whole(st.lbs, dy))
                fin = torch.isfinite(bnd)
                loose = bool(torch.any(torch.logical_and(~fin, dy.abs() > eps * N)))
                tot = float(torch.where(torch.logical_and(fin, dy != 0), bnd * dy, torch.zeros_like(dy)).sum())
                if st.m > 0:
                    tot += float((self._whole(st.bs, nu) * dnu).sum())
                c2 = float("inf") if loose else tot / N
            else:
                N = None
        self.checks.append((it, c1, c2, N, valid))
        return c1 is not None and c1 <= eps and c2 <= -eps

    def _dual(self, it, st, valid, prev, x, qx):
        eps = self.eps_dual_inf
        e1 = e2 = e3 = N = adx = None
        if valid:
            dx, dq = x - prev[5], qx - prev[6]
            N = float(dx.abs().max())
            if N > 0:
                e1 = float(dq.abs().max()) / N
                e2 = float((self._whole(st.ps, dx) * dx).sum()) / N
                zero = torch.zeros_like(dx)
                cone = torch.maximum(torch.where(torch.isfinite(self._whole(st.lbs, dx)), -dx, zero),
                                     torch.where(torch.isfinite(self._whole(st.ubs, dx)), dx, zero))
                e3 = max(float(cone.max()), 0.0) / N
                adx = float(torch.matmul(st.As, dx).abs().max()) / N if st.m > 0 else 0.0
            else:
                N = None
        self.dchecks.append((it, e1, e2, e3, N, valid))
        self.as_dx.append(adx)
        return e1 is not None and e1 <= eps and e2 <= -eps and e3 <= eps


def solve_with(cert, Q, p, A, b, lb, ub, control, bounds=None):
    """``oracle.solve_box_qp`` with the `Certificates` ``cert`` attached -> the oracle's dict plus "status" (0 optimal, 1 out of
    iterations, 2 primal infeasible, 3 dual infeasible), "n_factor" and the "checks" of cert"""
    trace = {}
    sol = O.solve_box_qp(Q, p, A, b, lb, ub, control, trace=trace, bounds=bounds, at_check=cert)
    sol.update(status=trace["status"], checks=cert.checks, n_factor=trace["n_factor"])
    return sol


def solve_detect(Q, p, A, b, lb, ub, control, eps_prim_inf=None, bounds=None, qx_from_rhs=False):
    """``oracle.solve_box_qp`` on a batch of ONE with the primal certificate at every check (eps_prim_inf=None: off, the oracle's
    bits).  -> the oracle's dict plus "status" (0 optimal, 1 out of iterations, 2 primal infeasible), "checks" (`Certificates`) and
    "n_factor"."""
    return solve_with(Certificates(eps_prim_inf, None, qx_from_rhs), Q, p, A, b, lb, ub, control, bounds)


@functools.lru_cache(maxsize=None)
def truth(name, dtype, detect=True):
    """-> every problem of the row solved by solve_detect as a batch of one (the bound flags of the whole batch: both finite)"""
    row = ROWS[name]
    qp = inputs(row, dtype)
    return [solve_detect(*E.alone(qp, i), control(row, problem=i), eps_prim_inf=EPS if detect else None, **E.ALONE)
            for i in range(row["B"])]


def margins_of(chk, flagged, miss, valid_at):
    """What the margins of both rules share, over the records `chk` of one solve, each (iteration, *terms, N, valid) with the
    validity flag at index `valid_at` -> (the terms of the flagged check, which is the last; None: not flagged,
    miss_before: miss(*terms) at the valid check before it; None: there is none,
    nearest: the smallest miss over the checks that did not flag; inf: never a valid snapshot with N > 0)."""
    terms = lambda c: c[1:valid_at - 1]
    last = miss_before = None
    if flagged:
        last = terms(chk[-1])
        if len(chk) > 1 and chk[-2][1] is not None:
            miss_before = miss(*terms(chk[-2]))
    nearest = min([miss(*terms(c)) for c in (chk[:-1] if flagged else chk) if c[1] is not None] or [float("inf")])
    return last, miss_before, nearest


def margins(sol, eps=EPS):
    """How far the rule is from its verdict over the checks of one solve -> (clear, miss_before, nearest):
    clear: min(eps / c1, -c2 / eps) at the detecting check (None: not flagged); miss_before: by what factor the rule missed at the
    valid check before it, max(c1 / eps, eps / max(-c2, 0)) (None: there is none); nearest: over the checks that did not flag, the
    smallest such miss (inf: never a valid snapshot)."""
    def miss(c1, c2):
        return max(c1 / eps, eps / max(-c2, 1e-300))
    last, miss_before, nearest = margins_of(sol["checks"], sol["status"] == INFEASIBLE, miss, 4)
    clear = None if last is None else min(eps / max(last[0], 1e-300), -last[1] / eps)
    return clear, miss_before, nearest


# (loop_kind, workgroups per problem) as last_forward_status names them: 2 the small loop, 1 the split loop, 0 the one-workgroup loop
SMALL, SPLIT2, SPLIT4, ONE = (2, 1), (1, 2), (1, 4), (0, 1)
_RHO1 = dict(E.THROUGH_EVENT, rho=1.)     # the event recipe with a given rho 100 times too small: the event at iteration 100 fires for every
                                          # problem that still runs, the infeasible ones among them -- they are detected BEHIND it

_row("small_n50", "small_n50_event", SMALL, gross=[4], mild=[2], control=E.PLAIN, q_scale=1., p_decades=5., seed=1,
     status=[0, 0, 2, 0, 2, 0, 0, 0], iters=[20, 40, 50, 40, 30, 10, 0, 0])
_row("split_n130", "split_n130", SPLIT2, gross=[2], mild=[5], seed=2, status=[0, 0, 2, 0, 0, 2, 0, 0], iters=[20, 60, 30, 40, 20, 50, 0, 0])
_row("split_n449", "split_n449", SPLIT4, gross=[1], mild=[2], seed=1, status=[0, 2, 2, 0, 0, 0, 0, 0], iters=[20, 40, 80, 60, 40, 20, 20, 0])
_row("split_n130_event", "split_n130_event", SPLIT2, gross=[0], mild=[2], f_mild=0.1, control=_RHO1, seed=1, status=[2, 0, 2, 0, 0, 0, 0, 0], iters=[120, 10, 140, 10, 0, 0, 0, 0])
# 17 equality rows: with f = 0.02 the certificate of row 0 converges by a few per cent per check and no seed holds the margin
_row("lu_n130_m17", "lu_n130_m17", ONE, gross=[4], mild=[1], f_mild=0.5, seed=1, status=[0, 2, 0, 0, 2, 0], iters=[30, 30, 40, 20, 30, 0])
_row("f64_n70_m3", "f64_n70_m3", ONE, gross=[3], mild=[0], seed=1, status=[2, 0, 0, 2, 0, 0, 0, 0], iters=[50, 50, 60, 30, 20, 10, 0, 0])
# The host-driven persistent schedule with a check at EVERY iteration.  The row's rho = 0.003 keeps two feasible problems running
# through the chunk boundaries; at that rho no certificate forms inside max_iters (float32 and float64 then disagree: the noise of
# c1 at k ~ 700 is the float32 limit DESIGN.md names), so the infeasible problems get a rho of their own, 1.0, and are flagged
# early.  From one iteration to the next c1 falls by a fifth at the most: no row of this kind can hold a factor 4 on both sides of
# a verdict.  1.1 is the widest factor both dtypes (and the form of Qs x that does not touch Q) give over the seeds tried.
_row("chunk_n20", "chunk_n20", ONE, gross=[3], mild=[4], margin=1.1, rho_b=[0.003, 0.003, 0.003, 1.0, 1.0, 0.003], seed=4,
     status=[1, 0, 0, 2, 2, 0], iters=[1199, 600, 0, 20, 36, 0])
# a batch of two cannot hold a gross, a mild and a feasible problem: one gross one, flagged behind its event, next to a feasible one
_row("big_n1030", "big_n1030", ONE, gross=[1], mild=[], control=dict(_RHO1, max_iters=400), seed=1, status=[0, 2], iters=[30, 150])
