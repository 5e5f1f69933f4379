"""The cases of the piecewise-linear layer -- min 0.5 x'Qx + p'x + sum_i f_i(x_i) over {Ax = b, lb <= x <= ub} with
f_i(x) = s_i0 x + sum_k (s_ik - s_i,k-1) (x - c_ik)_+, K <= 3 sorted kinks and K + 1 non-decreasing slopes per element -- and their truth
(no GPU needed to import this module).  tests/test_pwl_table.py checks them on the CPU, tests/test_gpu_pwl.py runs them.

The truth is `solve_pwl`: the oracle's iteration restated with one other z-update, on the oracle's own ``resolve_control``,
``equilibrate`` and ``kkt_matrix``, exactly as ``l1_table.solve_l1`` and ``soft_table.solve_soft`` are.  In the scaled space of the loop
(x = D xs) the data are ss_k = D s_k, cs_k = c_k / D, and with v = xh + u, t_k = ss_k / rho (true divisions, the rho of this iteration)
the step scans the kinks from the top, in exactly this compare form:

    for k = K .. 1:  d = v - cs_k;  S = v - t_k if d > t_k;  S = cs_k if d >= t_{k-1}
    S = v - t_0 otherwise            (S = v by a branch in front when every slope is zero);     z = min(max(S, lbs), ubs)

r, s, u, the six norms of a check and the rho events are the oracle's lines.  With K = 1 and slopes (-w, w) it returns solve_l1's x,
z, u, u_box bit for bit, with K = 2 and slopes (-wl, 0, wu) solve_soft's, with zero slopes the oracle's (test_pwl_table.py).  Behind the
loop the scan is taken once more at the returned iterate (v = z + u): piece = 2k on the slope s_k, 2k - 1 exactly on kink k -- only
where the kink's jump t_k - t_{k-1} is positive, else the element belongs to the piece below, 2k - 2 -- u_box = (S - clamp(S)) / D, and
lams is built from u_box.

`grad_recipe` is the backward: the kink set k is (piece == 2k - 1) without the elements a hard bound holds (u_box != 0), the effective
box (lb_e, ub_e) = on ? (c_k, c_k) : (lb, ub) with u_e = on ? u : u_box into the oracle's ``solve_box_qp_grad``, then dlb = dub = 0 on
the kink sets, dc_k = dlb_e + dub_e on kink set k, ds_k = dp on piece == 2k.

The pinned rows are l1_table's tier rows (``tier_table`` records, the same K, alpha and signatures) with three kinks on top: the kinks
(lo, c, hi) of soft_table.soft_data, the slopes (-(w0 + wl), -w0, w1, w1 + wu) with w0, w1 uniform in W01 -- turnover cost around c and
soft limits at lo, hi in one term -- and five kinds more: the user's K = 1 (the L1 term), the user's K = 2 with a middle slope 0 (the
band), a zero jump at the middle kink on half the elements, a kink on a hard bound, every hard bound infinite.
"""
import functools
import math

import torch

from oracle import boxqp_oracle as O
import l1_table as LT
import soft_table as ST
import tier_table as T

K_FAR, K_NEAR, K_EVENT = LT.K_FAR, LT.K_NEAR, LT.K_EVENT
PWL_K = 3
W01 = (0.02, 0.32)  # w0, w1: the slopes next to the middle kink
SHARE = 0.02        # every set of every sampled problem holds at least this share of the elements (n >= 129; n = 31: of the row)

TIERS = [(name, what.replace("FormL1", "FormPwl").replace("L1 instance", "piecewise-linear instance")) for name, what in LT.TIERS]
EVENT_ROW = LT.EVENT_ROW


def _row(name, K, what, kind="plain", alpha=1.0, j=0):
    """j: the seed offset (tier_table.seed_of) a search found -- the first at which every set of every sampled problem holds SHARE"""
    return dict(LT._row(name, K, what, alpha=alpha, j=j), pwl=kind, soft="hibound" if kind == "hibound" else "plain", l1="plain")


ROWS = {}
for _name, _what in TIERS:
    for _K in (K_FAR, K_NEAR):
        ROWS[f"{_name}-K{_K}"] = _row(_name, _K, _what, alpha=LT.ALPHA if _name in LT.RELAXED else 1.0)
ROWS[f"{EVENT_ROW}-K{K_EVENT}"] = _row(EVENT_ROW, K_EVENT, "hot / tail forms of the split loop around an adaptive-rho event: the t_k change with rho", j=6)
# (every other row's search ends at j = 0; the smallest set of a sampled problem, one of the two inner slopes, holds 0.020 to 0.056)
# above 1024 rows a thread of the streaming body owns a second element: its thresholds and kinks come back from the workspace
ROWS["wide_n1025_f32-K10"] = _row("wide_n1025_f32", K_FAR, "k_admm_loop<.., FormPwl>, LU branch, n > 1024: the t_k regions of the workspace are read")
ROWS["l1eq_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "the user's K = 1, slopes (-w, w): the L1 term", kind="l1eq")
ROWS["bandeq_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "the user's K = 2, slopes (-wl, 0, wu): the soft band", kind="bandeq")
ROWS["flat_n330-K60"] = _row("loop_split0_n330", K_NEAR, "a zero jump at the middle kink on half the elements", kind="flat")
ROWS["hibound_n31-K60"] = _row("small_n31_m1", K_NEAR, "hi_i = ub_i or lo_i = lb_i on some elements", kind="hibound")
ROWS["allinf_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "every hard bound infinite: the loop schedule all the same", kind="allinf")

SAME_BITS = LT.SAME_BITS
# l1eq / bandeq on the device against the L1 / soft-band kernels: one small, one split, one streaming LU float64 row
EQ_ROWS = ("small_n31_m1", "sweep2_n129_m1", "lu1_n300_f64")
GRAD_ROWS = {"sweep2_n129_m1": _row("sweep2_n129_m1", K_NEAR, "gradients, split loop"),
             "lu1_n300_f64": _row("lu1_n300_f64", K_NEAR, "gradients, streaming LU float64")}
GRADS8 = ("dQ", "dp", "dA", "db", "dlb", "dub", "ds", "dc")
OUTPUTS = T.OUTPUTS + ("piece", "u_box")
PIECES = tuple(range(2 * PWL_K + 1))
# the sets a kind empties by construction (the share is not asked of them)
EMPTY = {"l1eq": ("p3", "p4", "p5", "p6"), "bandeq": ("p5", "p6"), "allinf": ("clamped",)}

STOP, STOP_CONTROL, STOP_ROW = LT.STOP, LT.STOP_CONTROL, LT.STOP_ROW


def _inner(g, *shape):
    return W01[0] + (W01[1] - W01[0]) * torch.rand(*shape, generator=g, dtype=torch.float64)


def pwl_data(r, i, lb, ub):
    """(s, c) of problem i of row r, float64 (n, K + 1) and (n, K): K = 3 but for the kinds l1eq (1) and bandeq (2)"""
    n = r["n"]
    wl, wu, lo, hi = ST.soft_data(r, i, lb, ub)
    _, c = LT.l1_data(dict(r, l1="plain"), i, lb, ub)
    g = torch.Generator().manual_seed(T.seed_of(r) * 32452843 + 41 * i + 13)
    w0, w1 = _inner(g, n, 1), _inner(g, n, 1)
    kind = r.get("pwl", "plain")
    if kind == "l1eq":
        return torch.cat((-wl, wl), 1), c
    if kind == "bandeq":
        return torch.cat((-wl, torch.zeros_like(wl), wu), 1), torch.cat((lo, hi), 1)
    if kind == "flat":
        w0[0::2] = 0.0
        w1[0::2] = 0.0
    return torch.cat((-(w0 + wl), -w0, w1, w1 + wu), 1), torch.cat((lo, c, hi), 1)


def pwl_inputs(r, B, idx=None):
    """(Q, p, A, b, lb, ub, s, c) of the batch -- or of the problems `idx` of it -- in the row's dtype"""
    dt = torch.float32 if r["dtype"] == "f32" else torch.float64
    idx = list(range(B)) if idx is None else list(idx)
    base = [None if t is None else t.double() for t in T.inputs(dict(r, dtype="f64"), B, idx)]
    if r.get("pwl") == "allinf":
        base[4] = torch.full_like(base[4], -math.inf)
        base[5] = torch.full_like(base[5], math.inf)
    sc = [pwl_data(r, i, base[4][k], base[5][k]) for k, i in enumerate(idx)]
    base += [torch.stack([x[j] for x in sc]) for j in range(2)]
    return tuple(None if t is None else t.to(dt) for t in base)      # (rounding to float32 is monotone: sorted stays sorted)


def pad(s, c, K=PWL_K):
    """The same term with K kinks: kinks at +inf and the last slope repeated, at the top"""
    k = c.shape[2]
    return (torch.cat([s] + [s[:, :, -1:]] * (K - k), 2), torch.cat([c] + [torch.full_like(c[:, :, :1], math.inf)] * (K - k), 2))


def _cols(t):
    return [t[:, :, k:k + 1] for k in range(t.shape[2])]


def prox(v, t, cs):
    """S of the step, in exactly its compare form: t = [t_0 .. t_K], cs = [cs_1 .. cs_K], scanned from the top"""
    out = v - t[0]
    for k in range(1, len(t)):          # (built from the bottom: the outermost comparison is the top kink's)
        d = v - cs[k - 1]
        out = torch.where(d > t[k], v - t[k], torch.where(d >= t[k - 1], cs[k - 1] + torch.zeros_like(v), out))
    zero = functools.reduce(torch.logical_and, [tk == 0 for tk in t])
    return torch.where(zero, v, out)


def piece_of(v, t, cs):
    """where the scan ends: 2k on the slope s_k, 2k - 1 on kink k where its jump is positive, else the piece below it"""
    one = torch.ones_like(v)
    out = 0 * one
    for k in range(1, len(t)):
        d = v - cs[k - 1]
        out = torch.where(d > t[k], 2 * k * one, torch.where(d >= t[k - 1], torch.where(t[k] > t[k - 1], (2 * k - 1) * one, (2 * k - 2) * one), out))
    return out


def solve_pwl(Q, p, A, b, lb, ub, s, c, control, alpha=1.0, trace=None, step="pwl"):
    """The oracle's forward (oracle.solve_box_qp: same operations, same order) with the piecewise-linear step; returns its dict plus
    "piece", "u_box", and "lams" built from u_box.  step = "plain" / "band": the iterate of a kernel that ignores the term / the middle
    kink (the outer kinks with the outer slopes and 0 between them) -- what the rows must be far from."""
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
    ss, cs = [D * sk for sk in _cols(s)], [ck / D for ck in _cols(c)]
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
        if step == "pwl":
            S = prox(v, [sk / rho for sk in ss], cs)
        elif step == "band":
            S = prox(v, [ss[0] / rho, 0 * ss[0] / rho, ss[-1] / rho], [cs[0], cs[-1]])
        else:
            S = v
        z = torch.minimum(torch.maximum(S, lbs), ubs)
        r = x - z
        sres = rho * (z - z_old)
        u = u + (r if alpha == 1.0 else xh - z)
        if it % cr.check_solved == 0:
            r_inf = O._inf_norm_cols(D * r)
            s_inf = O._inf_norm_cols(D * sres)
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
    # ---- the scan once more at the returned iterate, in the scaled space (z == cs_k by assignment on a kink)
    v = z + u
    t = [sk / rho + torch.zeros_like(v) for sk in ss]
    piece = piece_of(v, t, cs)
    S = prox(v, t, cs)
    u_box = (S - torch.minimum(torch.maximum(S, lbs), ubs)) / D      # (S - z with the clamp taken again: exactly zero off the bounds)
    # "margin": how far every element is from changing its set -- the two comparisons at every kink and the distance from S to the
    # nearer bound, unscaled (a comparison with an infinite kink is infinitely far)
    margin = (S - lbs).abs().minimum((S - ubs).abs())
    for k in range(1, len(t)):
        d = v - cs[k - 1]
        margin = torch.minimum(margin, torch.minimum((d - t[k]).abs(), (d - t[k - 1]).abs()))
    margin = margin * D
    x, z, u = D * x, D * z, u / D
    y = u_box * rho
    lams = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    nus = xv[:, -m:, :] * E if m > 0 else None
    if trace is not None:
        trace.update(n_factor=n_factor)
    return {"x": x, "z": z, "u": u, "lams": lams, "nus": nus, "rho": rho, "iter": it, "piece": piece, "u_box": u_box, "margin": margin,
            "n_factor": n_factor}


def sets(sol):
    """-> {"p0" .. "p6": the seven pieces, unclamped; "clamped"}: bool (B, n, 1) each, a partition"""
    clamped = sol["u_box"] != 0
    out = {f"p{k}": (sol["piece"] == k) & ~clamped for k in PIECES}
    out["clamped"] = clamped
    return out


def truth(r, inp, dtype, step="pwl"):
    """The truth of row r on `inp` (eight tensors) in `dtype`, pinned to the row's K"""
    d = [None if t is None else t.to(dtype) for t in inp]
    return solve_pwl(*d, O.make_control(**T.control(r)), alpha=r["alpha"], step=step)


@functools.lru_cache(maxsize=None)
def row_truth(key, cus, table="ROWS"):
    """-> (idx, t32 or None, t64) of a row at `cus` compute units: the problems `tier_table.sample` picks, computed once and shared"""
    r = globals()[table][key]
    B = T.batch(r, cus)
    idx = T.sample(B)
    sub = pwl_inputs(r, B, idx)
    t64 = truth(r, sub, torch.float64)
    t32 = truth(r, sub, torch.float32) if r["dtype"] == "f32" else None
    return idx, t32, t64


def grad_recipe(cot, sol, Q, A, lb, ub, c):
    """The eight gradients of `cot` at the solution `sol` of solve_pwl: the effective box into the oracle's fixed-point backward;
    ds (B, n, K + 1) and dc (B, n, K) in the K of `c`"""
    piece = sol["piece"]
    K = c.shape[2]
    on = (piece % 2 == 1) & (sol["u_box"] == 0)      # (a kink beyond a hard bound: the bound holds the element, it is an ordinary clamped one)
    kv = torch.gather(c, 2, (((piece + 1) / 2).long() - 1).clamp(0, K - 1))
    lb_e, ub_e = torch.where(on, kv, lb), torch.where(on, kv, ub)
    u_e = torch.where(on, sol["u"], sol["u_box"])
    y = sol["rho"] * u_e
    lams_e = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    dQ, dp, dA, db, dlb_e, dub_e, _ = O.solve_box_qp_grad(cot, sol["x"], u_e, lams_e, sol["nus"], Q, A, lb_e, ub_e, sol["rho"])
    zero = torch.zeros_like(dp)
    return dict(dQ=dQ, dp=dp, dA=dA, db=db, dlb=torch.where(on, zero, dlb_e), dub=torch.where(on, zero, dub_e),
                ds=torch.cat([torch.where(piece == 2 * k, dp, zero) for k in range(K + 1)], 2),
                dc=torch.cat([torch.where(on & (piece == 2 * k - 1), dlb_e + dub_e, zero) for k in range(1, K + 1)], 2))


def truth_grads(r, inp, sol, cot, dtype):
    d = [None if t is None else t.to(dtype) for t in inp]
    return grad_recipe(cot.to(dtype), sol, d[0], d[2], d[4], d[5], d[7])


cot_of = LT.cot_of


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = ST.stop_inputs(torch.float64)
    wl, wu, lo, hi = qp[6:10]
    c = LT.stop_inputs(torch.float64)[7]
    g = torch.Generator().manual_seed(seed + 37)
    w0, w1 = _inner(g, B, n, 1), _inner(g, B, n, 1)
    s, k = torch.cat((-(w0 + wl), -w0, w1, w1 + wu), 2), torch.cat((lo, c, hi), 2)
    return tuple(None if t is None else t.to(dtype) for t in qp[:6] + (s, k))


@functools.lru_cache(maxsize=None)
def stop_truth(dtype):
    """The truth of a solve that stops by itself"""
    return solve_pwl(*stop_inputs(dtype), O.make_control(**STOP_CONTROL))


def excused(t64, bar_z):
    """bool (B, n, 1): elements whose `piece` may differ from the float64 truth's -- in that truth they sit within the bar for z of a
    comparison of the scan or of a bound"""
    return t64["margin"] < bar_z
