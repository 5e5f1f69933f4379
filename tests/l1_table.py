"""The cases of the L1 layer -- min 0.5 x'Qx + p'x + sum_i w_i |x_i - c_i| over {Ax = b, lb <= x <= ub} -- and their truth (no GPU
needed to import this module).  tests/test_l1_table.py checks them on the CPU, tests/test_gpu_l1.py runs them.

The truth is `solve_l1`: the oracle's iteration (``oracle.solve_box_qp``, the loop the reference-made goldens pin) restated with
one other z-update, on the oracle's own ``resolve_control``, ``equilibrate`` and ``kkt_matrix``.  In the scaled space of the loop
(x = D xs) the data are ws = D w, cs = c / D, and with v = xh + u, t = ws / rho (a true division, the rho of this iteration),
d = v - cs

    S = v - t if d > t,  v + t if d < -t,  cs otherwise;     z = min(max(S, lbs), ubs)

r, s, u, the six norms of a check and the rho events are the oracle's lines.  With w = 0 it returns the oracle's x, z, u, rho, iter
bit for bit (test_l1_table.py).  The solve always takes the loop schedule -- bounds that are all infinite are an ordinary case.
Behind the loop the step is evaluated once more at the returned iterate (v = z + u): side = sign(S - cs), 0 exactly on the kink
set K (the "otherwise" branch with t > 0), u_box = (S - clamp(S)) / D, the box's share of the dual (S - z with the clamp taken
again at this v, so that it is exactly zero unless the element is clamped), and lams is built from u_box.

`grad_recipe` is the backward: the effective box (lb_e, ub_e) = K ? (c, c) : (lb, ub) with u_e = K ? u : u_box into the oracle's
``solve_box_qp_grad``, then dlb = dub = 0 and dc = dlb_e + dub_e on K, dw = side * dp.

The pinned rows are records of ``tier_table.row`` with the L1 data on top (`l1_inputs`), so ``tier_table.batch / sample / control /
compare`` apply with their bars.  One row per kernel family that carries the step, at the shape and signature of the tier row it
is named after, at K = 10 (far from the fixed point) and K = 60; the event row at K = 110, just past its adaptive-rho event at
iteration 100, where t changes with rho.  The two dense-tier rows must land on the streaming body (the selector reroutes them):
their signature says one workgroup per problem.  One row above 1024 rows, where a thread of the streaming body owns two elements
and reads the second one's t back from the workspace.  Three rows more: every bound infinite, w = 0 on half the elements, c on a bound.
"""
import functools
import math

import torch

from oracle import boxqp_oracle as O
import tier_table as T

K_FAR, K_NEAR, K_EVENT = 10, 60, 110
ALPHA = 1.6
# the scale of w and c: w_i uniform in W_RANGE, c_i normal with deviation C_DEV -- chosen (test_l1_table.py holds every sampled problem
# of every row to it) so that the kink set, the thresholded free set and the clamped set each hold at least a tenth of the elements
W_RANGE = (0.02, 0.8)
C_DEV = 0.5

# (tier row, what runs the step there)
TIERS = [
    ("small_n31_m1", "k_admm_loop_small<FormL1>"),
    ("sweep2_n129_m1", "k_admm_loop_split<.., FormL1>, two workgroups, persistent"),
    ("sweep4_n511_m0", "k_admm_loop_split<.., FormL1>, four workgroups"),
    ("turns_n449_half1", "k_admm_loop_split<.., FormL1>, one launch per check segment, pairs taking turns"),
    ("loop_split0_n330", "k_admm_loop<.., FormL1>: the streaming body's symmetric branch, one workgroup"),
    ("big_n513_m2", "k_admm_loop_np2<FormL1>: the streaming body's symmetric branch, two workgroups"),
    ("lu_nonsym_n300", "k_admm_loop<.., FormL1>: the streaming body's LU branch, float32 (the plain solve takes the dense tier here)"),
    ("lu1_n300_f64", "k_admm_loop<.., FormL1>: the streaming body's LU branch, float64, segmented launches"),
    ("dense_n200_f32", "rerouted: the dense tier has no L1 instance, the streaming LU body runs"),
    ("densew_n257_f64", "rerouted: the W-workgroup dense tier has no L1 instance, the streaming LU body runs"),
    ("mode1_n330", "launch_mode = 1: the streaming body once per check segment"),
    ("mode2_nosync_n330", "sync = False through the module: the whole schedule enqueued"),
]
EVENT_ROW = "events_lo_n330"
RELAXED = ("sweep2_n129_m1", "lu1_n300_f64")       # alpha = 1.6 on top
# the dense tiers' problems land on the streaming body: one workgroup per problem, whatever the tier row's signature says
REROUTED = {"dense_n200_f32": dict(loop_workgroups=1, loop_kind=0), "densew_n257_f64": dict(loop_workgroups=1, loop_kind=0),
            "lu_nonsym_n300": dict(loop_workgroups=1, loop_kind=0), "wide_n1025_f32": dict(loop_workgroups=1, loop_kind=0)}


def _row(name, K, what, kind="plain", alpha=1.0, j=0):
    r = dict(T.ROW_BY_NAME[name], K=K, alpha=alpha, flip=None, why=what, l1=kind, j=j)
    r["sig"] = {k: v for k, v in r["sig"].items() if k != "n_factor"}      # (the test compares the count with the truth's own)
    if name in REROUTED:
        r["sig"] = dict(r["sig"], **REROUTED[name])
    return r


ROWS = {}
for _name, _what in TIERS:
    for _K in (K_FAR, K_NEAR):
        ROWS[f"{_name}-K{_K}"] = _row(_name, _K, _what, alpha=ALPHA if _name in RELAXED else 1.0)
ROWS[f"{EVENT_ROW}-K{K_EVENT}"] = _row(EVENT_ROW, K_EVENT, "hot / tail forms of the split loop around an adaptive-rho event: t changes with rho")
# above 1024 rows a thread of the streaming body owns a second element: its t comes back from the workspace
ROWS["wide_n1025_f32-K10"] = _row("wide_n1025_f32", K_FAR, "k_admm_loop<.., FormL1>, LU branch, n > 1024: the t region of the workspace is read")
ROWS["allinf_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "every bound infinite: the loop schedule all the same", kind="allinf")
ROWS["halfw_n330-K60"] = _row("loop_split0_n330", K_NEAR, "w = 0 on half the elements", kind="halfw")
ROWS["cbound_n31-K60"] = _row("small_n31_m1", K_NEAR, "c_i equals a bound on some elements", kind="cbound")

# w = 0 through the new entry against the plain forward, bit for bit: small, split (two workgroups), streaming LU float64
SAME_BITS = ("small_n31_m1", "sweep2_n129_m1", "lu1_n300_f64")
# gradients through the module at K = 60: one split row, one streaming LU float64 row (test_l1_table.py: the float32 and the
# float64 truth have identical sets on the first; `j` is what the seed search found)
GRAD_ROWS = {"sweep2_n129_m1": _row("sweep2_n129_m1", K_NEAR, "gradients, split loop"),
             "lu1_n300_f64": _row("lu1_n300_f64", K_NEAR, "gradients, streaming LU float64")}
GRADS8 = ("dQ", "dp", "dA", "db", "dlb", "dub", "dw", "dc")
OUTPUTS = T.OUTPUTS + ("side", "u_box")

# a solve that stops by itself (eps 1e-5, the oracle's generator): (n, B, seed)
STOP = (100, 4, 0)
STOP_CONTROL = dict(eps_abs=1e-5, eps_rel=1e-5)
STOP_ROW = dict(dtype="f32", R=T.R_DEFAULT, F=T.F_DEFAULT)


def l1_data(r, i, lb, ub):
    """(w, c) of problem i of row r, float64 (n, 1)"""
    n = r["n"]
    g = torch.Generator().manual_seed(T.seed_of(r) * 104729 + 17 * i + 3)
    w = W_RANGE[0] + (W_RANGE[1] - W_RANGE[0]) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    c = C_DEV * torch.randn(n, 1, generator=g, dtype=torch.float64)
    # c stays inside the box (yesterday's holdings were feasible), at least a hair
    c = torch.minimum(torch.maximum(c, lb), ub)
    kind = r.get("l1", "plain")
    if kind == "halfw":
        w[0::2] = 0.0
    if kind == "cbound":
        lo, hi = torch.arange(0, n, 5), torch.arange(2, n, 5)
        lo, hi = lo[torch.isfinite(lb[lo, 0])], hi[torch.isfinite(ub[hi, 0])]
        c[lo] = lb[lo]
        c[hi] = ub[hi]
    return w, c


def l1_inputs(r, B, idx=None):
    """(Q, p, A, b, lb, ub, w, c) of the batch -- or of the problems `idx` of it -- in the row's dtype"""
    dt = torch.float32 if r["dtype"] == "f32" else torch.float64
    idx = list(range(B)) if idx is None else list(idx)
    base = [None if t is None else t.double() for t in T.inputs(dict(r, dtype="f64"), B, idx)]
    if r.get("l1") == "allinf":
        base[4] = torch.full_like(base[4], -math.inf)
        base[5] = torch.full_like(base[5], math.inf)
    wc = [l1_data(r, i, base[4][k], base[5][k]) for k, i in enumerate(idx)]
    base += [torch.stack([x[0] for x in wc]), torch.stack([x[1] for x in wc])]
    return tuple(None if t is None else t.to(dt) for t in base)


def shrink(v, t, cs):
    """S of the step, in exactly its branch form"""
    d = v - cs
    return torch.where(d > t, v - t, torch.where(d < -t, v + t, cs + torch.zeros_like(v)))


def solve_l1(Q, p, A, b, lb, ub, w, c, control, alpha=1.0, trace=None, at_iter=None):
    """The oracle's forward (oracle.solve_box_qp: same operations, same order) with the L1 step; returns its dict plus "side", "u_box",
    and "lams" built from u_box.  at_iter(it, v, t, cs): shown what the step thresholds, in the scaled space."""
    B, n = Q.shape[0], p.shape[1]
    m = 0 if A is None else A.shape[1]
    dt = p.dtype
    p_inf = O._inf_norm_cols(p)
    cr = O.resolve_control(control, n)
    rho = cr.rho
    if cr.scale:
        sp = O.equilibrate(Q, p, A, b, lb, ub, cr.beta, True)
    else:
        sp = O.ScaledProblem(Q, p, A, b, lb, ub, 1.0, 1.0)
    Qs, ps, As, bs, lbs, ubs, D, E = sp.Q, sp.p, sp.A, sp.b, sp.lb, sp.ub, sp.D, sp.E
    ws, cs = D * w, c / D
    if rho is None:
        rho = torch.linalg.matrix_norm(Qs, keepdim=True) / n ** 0.5
        rho = torch.clamp(rho, min=cr.rho_min, max=cr.rho_max)
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
    thr = torch.ones(1) * cr.adaptive_rho_threshold
    r_inf = s_inf = pri_scale = dua_scale = None
    wants_rho = cr.adaptive_rho
    xv = None
    it = 0
    for it in range(cr.max_iters):
        if (cr.adaptive_rho and it % cr.adaptive_rho_iter == 0 and 0 < it < cr.adaptive_rho_max_iter and bool(torch.any(wants_rho))):
            ratio = (torch.clamp(r_inf / pri_scale, min=O.TINY) / torch.clamp(s_inf / dua_scale, min=O.TINY)) ** 0.5
            if bool((ratio > cr.adaptive_rho_tol).sum() > 0) or bool((ratio < 1 / cr.adaptive_rho_tol).sum() > 0):
                rho = rho * torch.logical_not(wants_rho) + (rho * ratio) * wants_rho
                rho = torch.clamp(rho, min=cr.rho_min, max=cr.rho_max)
                M[:, :n, :n] = Qs + rho * eye
                LU, piv = torch.linalg.lu_factor(M)
                n_factor += 1
        rhs = -ps + rho * (z - u)
        if m > 0:
            rhs = torch.cat((rhs, bs), 1)
        xv = torch.linalg.lu_solve(LU, piv, rhs)
        x = xv[:, :n, :]
        z_old = z
        xh = x if alpha == 1.0 else alpha * x + (1 - alpha) * z_old
        v = xh + u
        t = ws / rho
        if at_iter is not None:
            at_iter(it, v, t, cs)
        z = torch.minimum(torch.maximum(shrink(v, t, cs), lbs), ubs)
        r = x - z
        s = rho * (z - z_old)
        u = u + (r if alpha == 1.0 else xh - z)
        if it % cr.check_solved == 0:
            r_inf = O._inf_norm_cols(D * r)
            s_inf = O._inf_norm_cols(D * s)
            x_inf = O._inf_norm_cols(D * x)
            z_inf = O._inf_norm_cols(D * z)
            y_inf = O._inf_norm_cols(rho * D * u)
            qx_inf = O._inf_norm_cols(torch.matmul(Qs, x) / D)
            pri_scale = torch.maximum(torch.maximum(x_inf, z_inf), tiny)
            tol_p = cr.eps_abs + cr.eps_rel * pri_scale
            dua_scale = torch.maximum(torch.maximum(torch.maximum(y_inf, qx_inf), p_inf), tiny)
            tol_d = cr.eps_abs + cr.eps_rel * dua_scale
            solved = torch.logical_and(r_inf < tol_p, s_inf < tol_d)
            wants_rho = torch.logical_or(r_inf > torch.maximum(tol_p, thr), s_inf > torch.maximum(tol_d, thr))
            if torch.all(solved).item():
                break
    # ---- the step once more at the returned iterate, in the scaled space (z == cs by assignment on the kink)
    v = z + u
    t = ws / rho + torch.zeros_like(v)
    d = v - cs
    kink = (t > 0) & ~(d > t) & ~(d < -t)
    side = torch.where(kink, torch.zeros_like(v), torch.where(d < 0, -torch.ones_like(v), torch.ones_like(v)))
    S = shrink(v, t, cs)
    u_box = (S - torch.minimum(torch.maximum(S, lbs), ubs)) / D      # (S - z with the clamp taken again: exactly zero off the bounds)
    margin = torch.minimum((d.abs() - t).abs() * D, ((shrink(v, t, cs) - lbs).abs().minimum((shrink(v, t, cs) - ubs).abs())) * D)
    x, z, u = D * x, D * z, u / D
    y = u_box * rho
    lams = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    nus = xv[:, -m:, :] * E if m > 0 else None
    if trace is not None:
        trace.update(n_factor=n_factor)
    # "margin": how far every element is from changing its set -- | |d| - t | and the distance from S to the nearer bound, unscaled
    return {"x": x, "z": z, "u": u, "lams": lams, "nus": nus, "rho": rho, "iter": it, "side": side, "u_box": u_box, "margin": margin,
            "n_factor": n_factor}


def sets(sol):
    """-> (kink, thresholded free, clamped): bool (B, n, 1) each, a partition"""
    kink = sol["side"] == 0
    clamped = ~kink & (sol["u_box"] != 0)
    return kink, ~kink & ~clamped, clamped


def truth(r, inp, dtype, w_zero=False):
    """The truth of row r on `inp` (eight tensors) in `dtype`, pinned to the row's K"""
    d = [None if t is None else t.to(dtype) for t in inp]
    if w_zero:
        d[6] = torch.zeros_like(d[6])
    return solve_l1(*d, O.make_control(**T.control(r)), alpha=r["alpha"])


@functools.lru_cache(maxsize=None)
def row_truth(key, cus, table="ROWS"):
    """-> (idx, t32 or None, t64) of a row at `cus` compute units: the problems `tier_table.sample` picks, computed once and shared"""
    r = globals()[table][key]
    B = T.batch(r, cus)
    idx = T.sample(B)
    sub = l1_inputs(r, B, idx)
    t64 = truth(r, sub, torch.float64)
    t32 = truth(r, sub, torch.float32) if r["dtype"] == "f32" else None
    return idx, t32, t64


def grad_recipe(cot, sol, Q, A, lb, ub, c):
    """The eight gradients of `cot` at the solution `sol` of solve_l1: the effective box into the oracle's fixed-point backward"""
    n = Q.shape[1]
    K = sol["side"] == 0
    lb_e, ub_e = torch.where(K, c, lb), torch.where(K, c, ub)
    u_e = torch.where(K, sol["u"], sol["u_box"])
    y = sol["rho"] * u_e
    lams_e = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    dQ, dp, dA, db, dlb_e, dub_e, _ = O.solve_box_qp_grad(cot, sol["x"], u_e, lams_e, sol["nus"], Q, A, lb_e, ub_e, sol["rho"])
    zero = torch.zeros_like(dp)
    return dict(dQ=dQ, dp=dp, dA=dA, db=db, dlb=torch.where(K, zero, dlb_e), dub=torch.where(K, zero, dub_e),
                dw=sol["side"] * dp, dc=torch.where(K, dlb_e + dub_e, zero))


def truth_grads(r, inp, sol, cot, dtype):
    Q, _, A, _, lb, ub, _, c = [None if t is None else t.to(dtype) for t in inp]
    return grad_recipe(cot.to(dtype), sol, Q, A, lb, ub, c)


def cot_of(r, B, dtype):
    g = torch.Generator().manual_seed(T.seed_of(r) + 1)
    return torch.randn(B, r["n"], 1, generator=g, dtype=torch.float64).to(dtype)


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = O.create_qp_data(n, B, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 11)
    w = W_RANGE[0] + (W_RANGE[1] - W_RANGE[0]) * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    c = torch.minimum(torch.maximum(C_DEV * torch.randn(B, n, 1, generator=g, dtype=torch.float64), qp[4]), qp[5])
    return tuple(None if t is None else t.to(dtype) for t in qp + (w, c))


@functools.lru_cache(maxsize=None)
def stop_truth(dtype):
    """The truth of a solve that stops by itself"""
    return solve_l1(*stop_inputs(dtype), O.make_control(**STOP_CONTROL))


def excused(t64, bar_z):
    """bool (B, n, 1): elements whose `side` may differ from the float64 truth's -- their | |d| - t | or the distance from S to a
    bound, in that truth, is below the bar for z"""
    return t64["margin"] < bar_z
