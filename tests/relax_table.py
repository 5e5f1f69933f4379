"""The cases of control['alpha'], the over-relaxed ADMM step, and their truth (no GPU needed to import this module).
tests/test_relax_table.py checks them on the CPU, tests/test_gpu_relax.py runs them.

The truth is `solve_relaxed`: the loop of ``oracle.solve_box_qp`` restated with the relaxed step

    xh = alpha x + (1 - alpha) z_prev;  z = clamp(xh + u);  r = x - z;  s = rho (z - z_prev);  u = u + (xh - z)

on the oracle's own ``resolve_control``, ``equilibrate``, ``kkt_matrix`` and ``_inf_norm_cols``; at alpha = 1 it gives the oracle's
bits (test_relax_table.py).  Everything else of an iteration -- right-hand side, the six norms of a check with x_inf taken from x,
the rho events, the returned x -- is the oracle's.

The pinned rows are records of ``tier_table.row`` with an ``alpha`` on top, so ``tier_table.inputs / batch / sample / control /
compare`` apply with their bars: float32 |hip - t64| <= R |t32 - t64| + F scale (R = 4, F = 1e-7), float64 1e-9 scale, where t32 /
t64 are the RELAXED truth in float32 / float64.  One row per place the step is written and per kernel family, at the shape of the
tier row it is named after (the smallest at which that kernel can go wrong), with that row's signature.  K = 10 instead of the
tier table's 60: at the fixed point x = z and the relaxation term vanishes, so a converged comparison proves little; at K = 10 the
plain iterates are thousands of bars away from the relaxed ones (test_relax_table.py holds every row to 100 bars at the least).
The event row runs to K = 110, just past its adaptive-rho event at iteration 100.
"""
import functools

import torch

from oracle import boxqp_oracle as O
import each_table as E
import tier_table as T

K_PINNED, K_EVENT = 10, 110
ALPHA, ALPHA_UNDER = 1.6, 0.5

# (tier row, what runs the step there)
TIERS = [
    ("small_n31_m1", "k_admm_loop_small"),
    ("sweep2_n129_m1", "k_admm_loop_split, two workgroups, persistent"),
    ("sweep4_n511_m0", "k_admm_loop_split, four workgroups"),
    ("turns_n449_half1", "k_admm_loop_split, one launch per check segment, pairs taking turns"),
    ("loop_split0_n330", "k_admm_loop: the streaming body's symmetric branch, one workgroup"),
    ("big_n513_m2", "k_admm_loop_np2: the streaming body's symmetric branch, two workgroups"),
    ("lu_nonsym_n300", "the streaming body's LU branch / the dense tier above 256 rows, float32"),
    ("lu1_n300_f64", "k_admm_loop: the streaming body's LU branch, float64, segmented launches"),
    ("dense_n200_f32", "k_admm_loop_dense, float32"),
    ("densew_n257_f64", "k_admm_loop_dense_w, float64"),
    ("mode1_n330", "launch_mode = 1: the streaming body once per check segment"),
    ("mode2_nosync_n330", "sync = False through the module: the whole schedule enqueued"),
    ("events_lo_n330", "hot / tail forms of the split loop around an adaptive-rho event"),
]
UNDER = ("small_n31_m1", "sweep2_n129_m1")       # alpha < 1 in addition: a wrong sign on 1 - alpha

ROWS = {}
for _name, _what in TIERS:
    for _a in (ALPHA,) + ((ALPHA_UNDER,) if _name in UNDER else ()):
        _k = K_EVENT if _name == "events_lo_n330" else K_PINNED
        ROWS[f"{_name}-a{_a}"] = dict(T.ROW_BY_NAME[_name], K=_k, alpha=_a, flip=None, why=_what)

# alpha = 1.0 against the key absent, bit for bit: small, split (two workgroups), streaming LU, dense float64
SAME_BITS = ("small_n31_m1", "sweep2_n129_m1", "lu1_n300_f64", "densew_n257_f64")
# gradients through the module at the tier table's K = 60 (test_relax_table.py: no active-set flip between the float32 and the
# float64 truth on these two)
GRAD_ROWS = {name: dict(T.ROW_BY_NAME[name], K=T.K_DEFAULT, alpha=ALPHA, flip=None) for name in ("sweep2_n129_m1", "dense_n200_f32")}

# stopping by itself (eps 1e-5, the oracle's generator): (n, B, seed) -> last iteration without the key, with alpha = 1.6
STOPS = {(100, 4, 0): (60, 40), (40, 4, 1): (50, 30)}
STOP_CONTROL = dict(eps_abs=1e-5, eps_rel=1e-5)
# the bar of the stopped solves: a tier row's float32 bar
STOP_ROW = dict(dtype="f32", R=T.R_DEFAULT, F=T.F_DEFAULT)

# control['stop'] = 'each': one row of tests/each_table.py, every problem against its own relaxed solve as a batch of one
EACH_ROW = "split_n130"


def solve_relaxed(Q, p, A, b, lb, ub, control, alpha=1.0, trace=None, bounds=None):
    """``oracle.solve_box_qp`` with the over-relaxed step; returns the same dict.  trace: n_factor / n_solve / n_check."""
    B, n = Q.shape[0], p.shape[1]
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
    n_factor, n_solve, n_check = 1, 0, 0
    x = torch.zeros(B, n, 1, dtype=dt)
    z = torch.zeros(B, n, 1, dtype=dt)
    u = torch.zeros(B, n, 1, dtype=dt)
    tiny = torch.ones(1) * O.TINY
    thr = torch.ones(1) * c.adaptive_rho_threshold
    r_inf = s_inf = pri_scale = dua_scale = None
    wants_rho = c.adaptive_rho
    xv = None
    it = 0
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
        n_solve += 1
        x = xv[:, :n, :]
        # ---- the relaxed step ----
        z_old = z
        xh = alpha * x + (1 - alpha) * z_old
        z = xh + u
        if has_lb:
            z = torch.maximum(z, lbs)
        if has_ub:
            z = torch.minimum(z, ubs)
        r = x - z
        s = rho * (z - z_old)
        u = u + (xh - z)
        # ---- the oracle's check ----
        if it % c.check_solved == 0:
            n_check += 1
            r_inf = O._inf_norm_cols(D * r)
            s_inf = O._inf_norm_cols(D * s)
            x_inf = O._inf_norm_cols(D * x)
            z_inf = O._inf_norm_cols(D * z)
            y_inf = O._inf_norm_cols(rho * D * u)
            qx_inf = O._inf_norm_cols(torch.matmul(Qs, x) / D)
            pri_scale = torch.maximum(torch.maximum(x_inf, z_inf), tiny)
            tol_p = c.eps_abs + c.eps_rel * pri_scale
            dua_scale = torch.maximum(torch.maximum(torch.maximum(y_inf, qx_inf), p_inf), tiny)
            tol_d = c.eps_abs + c.eps_rel * dua_scale
            solved = torch.logical_and(r_inf < tol_p, s_inf < tol_d)
            wants_rho = torch.logical_or(r_inf > torch.maximum(tol_p, thr), s_inf > torch.maximum(tol_d, thr))
            if torch.all(solved).item():
                break
    x = D * x
    z = D * z
    u = u / D
    y = u * rho
    lams = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    nus = xv[:, -m:, :] * E_ if m > 0 else None
    if trace is not None:
        trace.update(n_factor=n_factor, n_solve=n_solve, n_check=n_check)
    return {"x": x, "z": z, "u": u, "lams": lams, "nus": nus, "rho": rho, "iter": it}


def truth(r, inp, dtype, alpha=None):
    """The relaxed truth of row r on `inp` in `dtype`, pinned to the row's K (plus "n_factor"); alpha: the row's, unless given."""
    d = [None if t is None else t.to(dtype) for t in inp]
    trace = {}
    sol = solve_relaxed(*d, O.make_control(**T.control(r)), alpha=r["alpha"] if alpha is None else alpha, trace=trace)
    sol["n_factor"] = trace["n_factor"]
    return sol


@functools.lru_cache(maxsize=None)
def row_truth(key, cus, table="ROWS"):
    """-> (idx, t32 or None, t64) of a row at `cus` compute units: the problems `tier_table.sample` picks, computed once and shared"""
    r = globals()[table][key]
    B = T.batch(r, cus)
    idx = T.sample(B)
    sub = T.inputs(r, B, idx)
    t64 = truth(r, sub, torch.float64)
    t32 = truth(r, sub, torch.float32) if r["dtype"] == "f32" else None
    return idx, t32, t64


def truth_grads(r, inp, sol, cot, dtype, backward):
    """The oracle's backward (`fixed_point` | `kkt`) of `cot` at the solution `sol` of the relaxed truth, in `dtype`"""
    Q, _, A, _, lb, ub = [None if t is None else t.to(dtype) for t in inp]
    if backward == "kkt":
        g = O.solve_box_qp_grad_kkt(cot.to(dtype), sol["x"], sol["lams"], sol["nus"], Q, A, lb, ub)
    else:
        g = O.solve_box_qp_grad(cot.to(dtype), sol["x"], sol["u"], sol["lams"], sol["nus"], Q, A, lb, ub, sol["rho"])
    return dict(zip(T.GRADS, g[:4]))


def cot_of(r, B, dtype):
    g = torch.Generator().manual_seed(T.seed_of(r) + 1)
    return torch.randn(B, r["n"], 1, generator=g, dtype=torch.float64).to(dtype)


@functools.lru_cache(maxsize=None)
def stop_truth(n, B, seed, alpha, dtype):
    """The relaxed truth of a solve that stops by itself, on the oracle's generator"""
    qp = O.create_qp_data(n, B, seed=seed, dtype=dtype)
    return solve_relaxed(*qp, O.make_control(**STOP_CONTROL), alpha=alpha)


@functools.lru_cache(maxsize=None)
def each_truth(dtype, alpha=ALPHA):
    """Every problem of EACH_ROW solved relaxed as a batch of one (the bound flags of the whole batch: both finite)"""
    row = E.ROWS[EACH_ROW]
    qp = E.inputs(row, dtype)
    out = []
    for i in range(row["B"]):
        one = tuple(None if t is None else t[i:i + 1] for t in qp)
        out.append(solve_relaxed(*one, E.control(row), alpha=alpha, bounds=(True, True)))
    return out
