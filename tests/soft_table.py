"""The cases of the soft-band layer -- min 0.5 x'Qx + p'x + sum_i [wl_i (lo_i - x_i)_+ + wu_i (x_i - hi_i)_+] over {Ax = b, lb <= x <= ub}
-- and their truth (no GPU needed to import this module).  tests/test_soft_table.py checks them on the CPU, tests/test_gpu_soft.py
runs them.

The truth is `solve_soft`: the oracle's iteration restated with one other z-update, on the oracle's own ``resolve_control``,
``equilibrate`` and ``kkt_matrix``, exactly as ``l1_table.solve_l1`` is.  In the scaled space of the loop (x = D xs) the data are
wls = D wl, wus = D wu, los = lo / D, his = hi / D, and with v = xh + u, tl = wls / rho, tu = wus / rho (true divisions, the rho
of this iteration), dh = v - his, dl = v - los

    S = v - tu if dh > tu,  v + tl if dl < -tl,  min(max(v, los), his) otherwise;     z = min(max(S, lbs), ubs)

r, s, u, the six norms of a check and the rho events are the oracle's lines.  With lo = hi = c, wl = wu = w it returns solve_l1's
x, z, u, u_box bit for bit, with wl = wu = 0 the oracle's x, z, u (test_soft_table.py).  Behind the loop the step is evaluated once
more at the returned iterate (v = z + u): zone = +2 if dh > tu, -2 if dl < -tl, else +1 if v >= his and tu > 0, else -1 if
v <= los and tl > 0, else 0; u_box = (S - clamp(S)) / D, and lams is built from u_box.

`grad_recipe` is the backward: Kl = (zone == -1), Kh = (zone == +1), each without the elements a hard bound holds (u_box != 0: a
kink outside [lb, ub] -- lo, hi = c -+ BAND rand does leave the box -- where x rests on the bound, not on the kink), the effective
box (lb_e, ub_e) = K ? (kink, kink) : (lb, ub) with u_e = K ? u : u_box into the oracle's ``solve_box_qp_grad``, then dlb = dub = 0 on K, dlo / dhi = dlb_e + dub_e on Kl / Kh,
dwu = dp on zone == +2, dwl = -dp on zone == -2.

The pinned rows are l1_table's tier rows (``tier_table`` records, the same K, alpha and signatures) with the band's data on top,
and five kinds more: lo = hi with wl = wu (the L1 term), lo = -inf everywhere (a hinge), zero weights on half the elements, a
kink on a hard bound, every hard bound infinite.
"""
import functools
import math

import torch

from oracle import boxqp_oracle as O
import l1_table as LT
import tier_table as T

K_FAR, K_NEAR, K_EVENT = LT.K_FAR, LT.K_NEAR, LT.K_EVENT
BAND = 0.5          # lo, hi = c -+ BAND * rand
SHARE = 0.05        # every set of every sampled problem holds at least this share of the elements (n >= 129; n = 31: of the row)

TIERS = [(name, what.replace("FormL1", "FormSoft").replace("L1 instance", "soft instance")) for name, what in LT.TIERS]
EVENT_ROW = LT.EVENT_ROW


def _row(name, K, what, kind="plain", alpha=1.0, j=0):
    """j: the seed offset (tier_table.seed_of) a search found -- the first at which every set of every sampled problem holds SHARE"""
    # (the event row asks one thing more of its j, see below)
    return dict(LT._row(name, K, what, alpha=alpha, j=j), soft=kind, l1="allinf" if kind == "allinf" else "plain")


ROWS = {}
for _name, _what in TIERS:
    for _K in (K_FAR, K_NEAR):
        ROWS[f"{_name}-K{_K}"] = _row(_name, _K, _what, alpha=LT.ALPHA if _name in LT.RELAXED else 1.0)
ROWS[f"{EVENT_ROW}-K{K_EVENT}"] = _row(EVENT_ROW, K_EVENT, "hot / tail forms of the split loop around an adaptive-rho event: tl, tu change with rho", j=7)
# The event row's j.  Behind the event every output hangs on the adapted rho, a square root of a ratio of four inf-norms, and the
# bar is R times ONE float32 realisation's distance from the float64 truth.  That distance is not a stable figure at every seed: in
# float32 with one entry in a few of Q moved to its neighbouring float (a relative 2^-24), |rho32 - rho64| over the sampled problems
# was, at j = 0 .. 10 (float64 solves on the CPU, no GPU figure involved):
#   j       0        1        2        3        4        5        6        7        8        9        10
#   as is   1.1e-4   7.3e-6   2.2e-4   2.7e-5   4.3e-5   1.2e-4   2.4e-4   2.1e-4   3.6e-5   1.6e-4   1.3e-4
#   moved   4.3e-5   7.8e-6   1.3e-4   4.0e-5   3.7e-5   3.0e-5   2.7e-5   1.5e-4   3.7e-5   1.7e-4   1.7e-5
#   share   .048     .030     .033     .039     .039     .061     .039     .055     .033     .067     .055
# j = 7 is the first whose smallest set holds SHARE and whose two realisations agree within a factor of two (j = 5 holds SHARE, 4 x
# apart: a bar drawn from the smaller one asks float32 arithmetic for a quarter of its own scatter).
# above 1024 rows a thread of the streaming body owns a second element: its thresholds and kinks come back from the workspace
ROWS["wide_n1025_f32-K10"] = _row("wide_n1025_f32", K_FAR, "k_admm_loop<.., FormSoft>, LU branch, n > 1024: the tl / tu regions of the workspace are read")
ROWS["l1eq_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "lo = hi, wl = wu: the L1 term", kind="l1eq")
ROWS["onesided_n330-K60"] = _row("loop_split0_n330", K_NEAR, "lo = -inf everywhere: a hinge above hi", kind="onesided")
ROWS["halfw_n330-K60"] = _row("loop_split0_n330", K_NEAR, "wl = wu = 0 on half the elements", kind="halfw", j=8)          # (only the other half can rest on a kink)
ROWS["hibound_n31-K60"] = _row("small_n31_m1", K_NEAR, "hi_i = ub_i or lo_i = lb_i on some elements", kind="hibound")
ROWS["allinf_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "every hard bound infinite: the loop schedule all the same", kind="allinf")

SAME_BITS = LT.SAME_BITS
# l1eq on the device against the L1 kernels: one small, one split, one streaming LU float64 row
L1EQ_ROWS = ("small_n31_m1", "sweep2_n129_m1", "lu1_n300_f64")
GRAD_ROWS = {"sweep2_n129_m1": _row("sweep2_n129_m1", K_NEAR, "gradients, split loop"),
             "lu1_n300_f64": _row("lu1_n300_f64", K_NEAR, "gradients, streaming LU float64")}
GRADS10 = ("dQ", "dp", "dA", "db", "dlb", "dub", "dwl", "dwu", "dlo", "dhi")
OUTPUTS = T.OUTPUTS + ("zone", "u_box")
ZONES = (-2, -1, 0, 1, 2)
# the sets a kind empties by construction (the share is not asked of them)
EMPTY = {"l1eq": ("z0",), "onesided": ("z-2", "z-1"), "allinf": ("clamped",)}

STOP, STOP_CONTROL, STOP_ROW = LT.STOP, LT.STOP_CONTROL, LT.STOP_ROW


def soft_data(r, i, lb, ub):
    """(wl, wu, lo, hi) of problem i of row r, float64 (n, 1): c and w are l1_table.l1_data's, the band is c -+ BAND rand, wu is drawn
    independently in l1_table.W_RANGE"""
    n = r["n"]
    wl, c = LT.l1_data(dict(r, l1="plain"), i, lb, ub)
    g = torch.Generator().manual_seed(T.seed_of(r) * 15485863 + 31 * i + 7)
    lo = c - BAND * torch.rand(n, 1, generator=g, dtype=torch.float64)
    hi = c + BAND * torch.rand(n, 1, generator=g, dtype=torch.float64)
    wu = LT.W_RANGE[0] + (LT.W_RANGE[1] - LT.W_RANGE[0]) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    kind = r.get("soft", "plain")
    if kind == "l1eq":
        lo, hi, wu = c.clone(), c.clone(), wl.clone()
    if kind == "onesided":
        lo = torch.full_like(lo, -math.inf)
    if kind == "halfw":
        wl[0::2] = 0.0
        wu[0::2] = 0.0
    if kind == "hibound":
        il, ih = torch.arange(0, n, 5), torch.arange(2, n, 5)
        il, ih = il[torch.isfinite(lb[il, 0])], ih[torch.isfinite(ub[ih, 0])]
        lo[il] = lb[il]
        hi[il] = torch.maximum(hi[il], lb[il])
        hi[ih] = ub[ih]
        lo[ih] = torch.minimum(lo[ih], ub[ih])
    return wl, wu, lo, hi


def soft_inputs(r, B, idx=None):
    """(Q, p, A, b, lb, ub, wl, wu, lo, hi) of the batch -- or of the problems `idx` of it -- in the row's dtype"""
    dt = torch.float32 if r["dtype"] == "f32" else torch.float64
    idx = list(range(B)) if idx is None else list(idx)
    base = [None if t is None else t.double() for t in T.inputs(dict(r, dtype="f64"), B, idx)]
    if r.get("soft") == "allinf":
        base[4] = torch.full_like(base[4], -math.inf)
        base[5] = torch.full_like(base[5], math.inf)
    sd = [soft_data(r, i, base[4][k], base[5][k]) for k, i in enumerate(idx)]
    base += [torch.stack([x[j] for x in sd]) for j in range(4)]
    return tuple(None if t is None else t.to(dt) for t in base)      # (rounding to float32 is monotone: lo <= hi stays, lo == hi too)


def prox(v, tl, tu, los, his):
    """S of the step, in exactly its branch form"""
    dh, dl = v - his, v - los
    return torch.where(dh > tu, v - tu, torch.where(dl < -tl, v + tl, torch.minimum(torch.maximum(v, los), his)))


def solve_soft(Q, p, A, b, lb, ub, wl, wu, lo, hi, control, alpha=1.0, trace=None, step="soft"):
    """The oracle's forward (oracle.solve_box_qp: same operations, same order) with the soft band's step; returns its dict plus
    "zone", "u_box", and "lams" built from u_box.  step = "plain" / "l1": the iterate of a kernel that ignores the band / takes it for
    an L1 term around its middle -- what the rows must be far from."""
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
    wls, wus, los, his = D * wl, D * wu, lo / D, hi / D
    if step == "l1":
        l1w, l1c = D * ((wl + wu) / 2), ((lo + hi) / 2) / D
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
        if step == "soft":
            S = prox(v, wls / rho, wus / rho, los, his)
        elif step == "l1":
            S = LT.shrink(v, l1w / rho, l1c)
        else:
            S = v
        z = torch.minimum(torch.maximum(S, lbs), ubs)
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
    # ---- the step once more at the returned iterate, in the scaled space (z == his / los by assignment on a kink)
    v = z + u
    tl, tu = wls / rho + torch.zeros_like(v), wus / rho + torch.zeros_like(v)
    dh, dl = v - his, v - los
    one = torch.ones_like(v)
    zone = torch.where(dh > tu, 2 * one, torch.where(dl < -tl, -2 * one, torch.where((v >= his) & (tu > 0), one,
                       torch.where((v <= los) & (tl > 0), -one, 0 * one))))
    S = prox(v, tl, tu, los, his)
    u_box = (S - torch.minimum(torch.maximum(S, lbs), ubs)) / D      # (S - z with the clamp taken again: exactly zero off the bounds)
    # "margin": how far every element is from changing its set -- the four comparisons of the zone and the distance from S to the
    # nearer bound, unscaled (a comparison with an infinite kink is infinitely far)
    inf = torch.full_like(v, math.inf)
    margin = torch.minimum((dh - tu).abs(), (dl + tl).abs())
    margin = torch.minimum(margin, torch.where(tu > 0, dh.abs(), inf))
    margin = torch.minimum(margin, torch.where(tl > 0, dl.abs(), inf))
    margin = torch.minimum(margin, (S - lbs).abs().minimum((S - ubs).abs())) * D
    x, z, u = D * x, D * z, u / D
    y = u_box * rho
    lams = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    nus = xv[:, -m:, :] * E if m > 0 else None
    if trace is not None:
        trace.update(n_factor=n_factor)
    return {"x": x, "z": z, "u": u, "lams": lams, "nus": nus, "rho": rho, "iter": it, "zone": zone, "u_box": u_box, "margin": margin,
            "n_factor": n_factor}


def sets(sol):
    """-> {"z-2", "z-1", "z0", "z1", "z2": the five zones, unclamped; "clamped"}: bool (B, n, 1) each, a partition"""
    clamped = sol["u_box"] != 0
    out = {f"z{k}": (sol["zone"] == k) & ~clamped for k in ZONES}
    out["clamped"] = clamped
    return out


def truth(r, inp, dtype, step="soft", w_zero=False):
    """The truth of row r on `inp` (ten tensors) in `dtype`, pinned to the row's K"""
    d = [None if t is None else t.to(dtype) for t in inp]
    if w_zero:
        d[6], d[7] = torch.zeros_like(d[6]), torch.zeros_like(d[7])
    return solve_soft(*d, O.make_control(**T.control(r)), alpha=r["alpha"], step=step)


@functools.lru_cache(maxsize=None)
def row_truth(key, cus, table="ROWS"):
    """-> (idx, t32 or None, t64) of a row at `cus` compute units: the problems `tier_table.sample` picks, computed once and shared"""
    r = globals()[table][key]
    B = T.batch(r, cus)
    idx = T.sample(B)
    sub = soft_inputs(r, B, idx)
    t64 = truth(r, sub, torch.float64)
    t32 = truth(r, sub, torch.float32) if r["dtype"] == "f32" else None
    return idx, t32, t64


def grad_recipe(cot, sol, Q, A, lb, ub, lo, hi):
    """The ten gradients of `cot` at the solution `sol` of solve_soft: the effective box into the oracle's fixed-point backward"""
    zone = sol["zone"]
    free = sol["u_box"] == 0          # (a kink beyond a hard bound: the bound holds the element, it is an ordinary clamped one)
    Kl, Kh = (zone == -1) & free, (zone == 1) & free
    K = Kl | Kh
    kv = torch.where(Kh, hi, lo)
    lb_e, ub_e = torch.where(K, kv, lb), torch.where(K, kv, ub)
    u_e = torch.where(K, sol["u"], sol["u_box"])
    y = sol["rho"] * u_e
    lams_e = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    dQ, dp, dA, db, dlb_e, dub_e, _ = O.solve_box_qp_grad(cot, sol["x"], u_e, lams_e, sol["nus"], Q, A, lb_e, ub_e, sol["rho"])
    zero = torch.zeros_like(dp)
    return dict(dQ=dQ, dp=dp, dA=dA, db=db, dlb=torch.where(K, zero, dlb_e), dub=torch.where(K, zero, dub_e),
                dwl=torch.where(zone == -2, -dp, zero), dwu=torch.where(zone == 2, dp, zero),
                dlo=torch.where(Kl, dlb_e + dub_e, zero), dhi=torch.where(Kh, dlb_e + dub_e, zero))


def truth_grads(r, inp, sol, cot, dtype):
    d = [None if t is None else t.to(dtype) for t in inp]
    return grad_recipe(cot.to(dtype), sol, d[0], d[2], d[4], d[5], d[8], d[9])


cot_of = LT.cot_of


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = LT.stop_inputs(torch.float64)
    wl, c = qp[6], qp[7]
    g = torch.Generator().manual_seed(seed + 23)
    lo = c - BAND * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    hi = c + BAND * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    wu = LT.W_RANGE[0] + (LT.W_RANGE[1] - LT.W_RANGE[0]) * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    return tuple(None if t is None else t.to(dtype) for t in qp[:6] + (wl, wu, lo, hi))


@functools.lru_cache(maxsize=None)
def stop_truth(dtype):
    """The truth of a solve that stops by itself"""
    return solve_soft(*stop_inputs(dtype), O.make_control(**STOP_CONTROL))


def excused(t64, bar_z):
    """bool (B, n, 1): elements whose `zone` may differ from the float64 truth's -- in that truth they sit within the bar for z of a
    comparison of the zone or of a bound"""
    return t64["margin"] < bar_z
