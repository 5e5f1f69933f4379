"""The cases of control['infeasible'], primal infeasibility detection under control['stop'] = 'each', and their truth (no GPU
needed to import this module).  tests/test_infeas_table.py checks them on the CPU, tests/test_gpu_infeas.py runs them.

The truth is `solve_detect`: the loop of ``oracle.solve_box_qp`` restated for a batch of one (in the manner of
``relax_table.solve_relaxed``) with the certificate at every check.  In the SCALED problem, after the element-wise update of
iteration k:

    y = rho u_k;  g = Qs x_k + rho (z_k - z_{k-1});  nu = nu_k

against the snapshot (y, g, nu) of the last check, which is valid iff rho has not changed since:

    dy, dg, dnu;  N = |dy|_inf;  c1 = |dg|_inf / N;  c2 = (sum_i [ubs_i max(dy_i, 0) + lbs_i min(dy_i, 0)] + bs^T dnu) / N

(a term of an infinite bound counts 0 while |dy_i| <= eps N, else c2 = +inf) and "primal infeasible" iff N > 0, c1 <= eps and
c2 <= -eps.  Optimal comes first; a flagged problem stops with the iterate of that check.  With detection off it is the oracle,
bit for bit (test_infeas_table.py).

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
OPTIMAL, MAXITER, INFEASIBLE = 0, 1, 2

ROWS = {}


def _row(name, base, tier, gross, mild, status, iters, f_mild=0.02, margin=MARGIN, rho_b=None, **kw):
    """base: the each_table row it builds on (kw: what differs); tier: (loop_kind, workgroups per QP) as test_gpu_each.py asserts;
    f_mild: the f of the `mild` problems where 0.02 gives no row that holds the margin; rho_b: one given rho per problem"""
    row = dict(E.ROWS[base], **kw)
    row.update(name=name, tier=tier, gross=gross, mild=mild, status=status, iters=iters, f_mild=f_mild, margin=margin, rho_b=rho_b,
               infeasible_last=False, never=[], adapts=None)
    ROWS[name] = row


def inputs(row, dtype=torch.float64):
    """-> Q, p, A, b, lb, ub: each_table's inputs of the row with b_0 of the `gross` / `mild` problems moved out of reach"""
    Q, p, A, b, lb, ub = E.inputs(row, torch.float64)
    for idx, f in ((row["gross"], 1.0), (row["mild"], row.get("f_mild", 0.02))):
        for i in idx:
            a0 = A[i, 0]
            hi = float((a0 * torch.where(a0 > 0, ub[i, :, 0], lb[i, :, 0])).sum())
            lo = float((a0 * torch.where(a0 > 0, lb[i, :, 0], ub[i, :, 0])).sum())
            b[i, 0, 0] = hi + f * (hi - lo)
    cast = lambda t: None if t is None else t.to(dtype).contiguous()
    return tuple(cast(t) for t in (Q, p, A, b, lb, ub))


def control(row, problem=None, **extra):
    """the oracle's control of the row; problem: of that problem solved alone (rows with one rho per problem, `rho_b`)"""
    if problem is not None and row.get("rho_b") is not None:
        extra = dict(extra, rho=float(row["rho_b"][problem]))
    return O.make_control(**dict(row["control"], **extra))


def solve_detect(Q, p, A, b, lb, ub, control, eps_prim_inf=None, bounds=None, qx_from_rhs=False):
    """``oracle.solve_box_qp`` on a batch of ONE with the certificate at every check (eps_prim_inf=None: off, the oracle's bits).
    -> the oracle's dict plus "status" (0 optimal, 1 out of iterations, 2 primal infeasible) and "checks": per check
    (iteration, c1, c2, N, valid), c1 = c2 = N = None where there was no valid snapshot or N == 0.  qx_from_rhs: the certificate's
    Qs x is w - rho x - As^T nu, as a kernel that does not touch Q forms it, not the product (the rows' verdicts must not care)."""
    assert Q.shape[0] == 1
    B, n = 1, p.shape[1]
    m = O._ncon(A, 1)
    dt = p.dtype
    p_inf = O._inf_norm_cols(p)
    has_lb = bool(torch.max(lb) > -O.INF) if bounds is None else bool(bounds[0])
    has_ub = bool(torch.min(ub) < O.INF) if bounds is None else bool(bounds[1])
    has_box = has_lb or has_ub
    c = O.resolve_control(control, n)
    rho = c.rho
    if not has_box:
        rho = 0
    if c.scale:
        sp = O.equilibrate(Q, p, A, b, lb, ub, c.beta, has_box)
    else:
        sp = O.ScaledProblem(Q, p, A, b, lb, ub, 1.0, 1.0)
    Qs, ps, As, bs, lbs, ubs, D, E_ = sp.Q, sp.p, sp.A, sp.b, sp.lb, sp.ub, sp.D, sp.E
    if rho is None:
        rho = torch.linalg.matrix_norm(Qs, keepdim=True) / n ** 0.5
        rho = torch.clamp(rho, min=c.rho_min, max=c.rho_max)
    eye = torch.eye(n, dtype=dt).unsqueeze(0)
    M = Qs + rho * eye
    if m > 0:
        M = O.kkt_matrix(M, As, torch.zeros(B, m, m, dtype=dt))
    LU, piv = torch.linalg.lu_factor(M)
    n_factor = 1
    x = torch.zeros(B, n, 1, dtype=dt)
    z = torch.zeros(B, n, 1, dtype=dt)
    u = torch.zeros(B, n, 1, dtype=dt)
    tiny = torch.ones(1) * O.TINY
    thr = torch.ones(1) * c.adaptive_rho_threshold
    r_inf = s_inf = pri_scale = dua_scale = None
    wants_rho = c.adaptive_rho
    xv = None
    it = 0
    status = MAXITER
    snap = None              # (y, g, nu, rho it was taken at, iteration)
    checks = []
    lbs_b = torch.broadcast_to(torch.as_tensor(lbs, dtype=dt), (B, n, 1))
    ubs_b = torch.broadcast_to(torch.as_tensor(ubs, dtype=dt), (B, n, 1))
    for it in range(c.max_iters):
        if (c.adaptive_rho and it % c.adaptive_rho_iter == 0 and 0 < it < c.adaptive_rho_max_iter
                and bool(torch.any(wants_rho))):
            ratio = (torch.clamp(r_inf / pri_scale, min=O.TINY) / torch.clamp(s_inf / dua_scale, min=O.TINY)) ** 0.5
            grow = bool((ratio > c.adaptive_rho_tol).sum() > 0)
            shrink = bool((ratio < 1 / c.adaptive_rho_tol).sum() > 0)
            if grow or shrink:
                rho = rho * torch.logical_not(wants_rho) + (rho * ratio) * wants_rho
                rho = torch.clamp(rho, min=c.rho_min, max=c.rho_max)
                M[:, :n, :n] = Qs + rho * eye
                LU, piv = torch.linalg.lu_factor(M)
                n_factor += 1
        rhs = -ps + rho * (z - u)
        if m > 0:
            rhs = torch.cat((rhs, bs), 1)
        xv = torch.linalg.lu_solve(LU, piv, rhs)
        x = xv[:, :n, :]
        z_old = z
        z = x + u
        if has_lb:
            z = torch.maximum(z, lbs)
        if has_ub:
            z = torch.minimum(z, ubs)
        r = x - z
        s = rho * (z - z_old)
        u = u + r
        if it % c.check_solved == 0:
            r_inf = O._inf_norm_cols(D * r)
            s_inf = O._inf_norm_cols(D * s)
            x_inf = O._inf_norm_cols(D * x)
            z_inf = O._inf_norm_cols(D * z)
            y_inf = O._inf_norm_cols(rho * D * u)
            qx = torch.matmul(Qs, x)
            qx_inf = O._inf_norm_cols(qx / D)
            pri_scale = torch.maximum(torch.maximum(x_inf, z_inf), tiny)
            tol_p = c.eps_abs + c.eps_rel * pri_scale
            dua_scale = torch.maximum(torch.maximum(torch.maximum(y_inf, qx_inf), p_inf), tiny)
            tol_d = c.eps_abs + c.eps_rel * dua_scale
            solved = torch.logical_and(r_inf < tol_p, s_inf < tol_d)
            wants_rho = torch.logical_or(r_inf > torch.maximum(tol_p, thr), s_inf > torch.maximum(tol_d, thr))
            if torch.all(solved).item():
                status = OPTIMAL
                break
            if eps_prim_inf is not None:
                eps = eps_prim_inf
                rho_now = float(torch.as_tensor(rho).reshape(-1)[0])
                nu = xv[:, n:, :] if m > 0 else torch.zeros(B, 0, 1, dtype=dt)
                qx_c = qx
                if qx_from_rhs:
                    qx_c = rhs[:, :n, :] - rho * x - (torch.matmul(As.transpose(1, 2), nu) if m > 0 else 0)
                y, g = rho * u, qx_c + s
                valid = snap is not None and snap[3] == rho_now and snap[4] == it - c.check_solved
                c1 = c2 = N = None
                if valid:
                    dy, dg, dnu = y - snap[0], g - snap[1], nu - snap[2]
                    N = float(dy.abs().max())
                    if N > 0:
                        c1 = float(dg.abs().max()) / N
                        bnd = torch.where(dy > 0, ubs_b, lbs_b)
                        fin = torch.isfinite(bnd)
                        loose = bool(torch.any(torch.logical_and(~fin, dy.abs() > eps * N)))
                        tot = float(torch.where(torch.logical_and(fin, dy != 0), bnd * dy, torch.zeros_like(dy)).sum())
                        if m > 0:
                            tot += float((torch.broadcast_to(torch.as_tensor(bs, dtype=dt), nu.shape) * dnu).sum())
                        c2 = float("inf") if loose else tot / N
                    else:
                        N = None
                checks.append((it, c1, c2, N, valid))
                snap = (y.clone(), g.clone(), nu.clone(), rho_now, it)
                if c1 is not None and c1 <= eps and c2 <= -eps:
                    status = INFEASIBLE
                    break
    x = D * x
    z = D * z
    u = u / D
    y = u * rho
    lams = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    nus = xv[:, -m:, :] * E_ if m > 0 else None
    return {"x": x, "z": z, "u": u, "lams": lams, "nus": nus, "rho": rho, "iter": it, "status": status, "checks": checks,
            "n_factor": n_factor}


@functools.lru_cache(maxsize=None)
def truth(name, dtype, detect=True):
    """-> every problem of the row solved by solve_detect as a batch of one (the bound flags of the whole batch: both finite)"""
    row = ROWS[name]
    qp = inputs(row, dtype)
    out = []
    for i in range(row["B"]):
        one = tuple(None if t is None else t[i:i + 1] for t in qp)
        out.append(solve_detect(*one, control(row, problem=i), eps_prim_inf=EPS if detect else None, bounds=(True, True)))
    return out


def margins(sol, eps=EPS):
    """How far the rule is from its verdict over the checks of one solve -> (clear, miss_before, nearest):
    clear: min(eps / c1, -c2 / eps) at the detecting check (None: not flagged); miss_before: by what factor the rule missed at the
    valid check before it, max(c1 / eps, eps / max(-c2, 0)) (None: there is none); nearest: over the checks that did not flag, the
    smallest such miss (inf: never a valid snapshot)."""
    def miss(c1, c2):
        return max(c1 / eps, eps / max(-c2, 1e-300))
    chk = sol["checks"]
    flagged = sol["status"] == INFEASIBLE
    clear = miss_before = None
    body = chk[:-1] if flagged else chk
    if flagged:
        _, c1, c2, _, _ = chk[-1]
        clear = min(eps / max(c1, 1e-300), -c2 / eps)
        if len(chk) > 1 and chk[-2][1] is not None:
            miss_before = miss(chk[-2][1], chk[-2][2])
    nearest = min([miss(c1, c2) for _, c1, c2, _, _ in body if c1 is not None] or [float("inf")])
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
