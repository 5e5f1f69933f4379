"""The cases of the piecewise-linear layer -- min 0.5 x'Qx + p'x + sum_i f_i(x_i) over {Ax = b, lb <= x <= ub} with
f_i(x) = s_i0 x + sum_k (s_ik - s_i,k-1) (x - c_ik)_+, K <= 3 sorted kinks and K + 1 non-decreasing slopes per element -- and their truth
(no GPU needed to import this module).  tests/test_pwl_table.py checks them on the CPU, tests/test_gpu_pwl.py runs them.

The truth is `solve_pwl`: the oracle's own iteration (``oracle.solve_box_qp``) with `PwlTerm` as its ``term=`` -- the one other
z-update -- through the record `TERM` (tests/term_table.py), exactly as ``l1_table.solve_l1`` and ``soft_table.solve_soft`` are.  In the
scaled space of the loop
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
import term_table as TT
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


class PwlTerm:
    """sum_i f_i(x_i) for oracle.solve_box_qp(term=): ss_k = D s_k, cs_k = c_k / D, t_k = ss_k / rho"""

    def __init__(self, s, c):
        self.s, self.c = s, c

    def scale(self, D):
        self.ss, self.cs = [D * sk for sk in _cols(self.s)], [ck / D for ck in _cols(self.c)]

    def step(self, v, rho):
        return prox(v, [sk / rho for sk in self.ss], self.cs)

    def finish(self, z, u, rho, lbs, ubs, D):
        """the scan once more at the returned iterate, in the scaled space (z == cs_k by assignment on a kink)"""
        cs = self.cs
        v = z + u
        t = [sk / rho + torch.zeros_like(v) for sk in self.ss]
        piece = piece_of(v, t, cs)
        S = prox(v, t, cs)
        u_box = (S - torch.minimum(torch.maximum(S, lbs), ubs)) / D      # (S - z with the clamp taken again: exactly zero off the bounds)
        # "margin": how far every element is from changing its set -- the two comparisons at every kink and the distance from S to the
        # nearer bound, unscaled (a comparison with an infinite kink is infinitely far)
        margin = (S - lbs).abs().minimum((S - ubs).abs())
        for k in range(1, len(t)):
            d = v - cs[k - 1]
            margin = torch.minimum(margin, torch.minimum((d - t[k]).abs(), (d - t[k - 1]).abs()))
        return {"piece": piece, "u_box": u_box, "margin": margin * D}


class PwlPlain(PwlTerm):
    """the iterate of a kernel that ignores the term (the classification behind the loop is the term's all the same)"""

    def step(self, v, rho):
        return v


class PwlAsBand(PwlTerm):
    """the iterate of a kernel that ignores the middle kink: the outer kinks with the outer slopes and 0 between them"""

    def step(self, v, rho):
        ss, cs = self.ss, self.cs
        return prox(v, [ss[0] / rho, 0 * ss[0] / rho, ss[-1] / rho], [cs[0], cs[-1]])


def sets(sol):
    """-> {"p0" .. "p6": the seven pieces, unclamped; "clamped"}: bool (B, n, 1) each, a partition"""
    clamped = sol["u_box"] != 0
    out = {f"p{k}": (sol["piece"] == k) & ~clamped for k in PIECES}
    out["clamped"] = clamped
    return out


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


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = ST.stop_inputs(torch.float64)
    wl, wu, lo, hi = qp[6:10]
    c = LT.stop_inputs(torch.float64)[7]
    g = torch.Generator().manual_seed(seed + 37)
    w0, w1 = _inner(g, B, n, 1), _inner(g, B, n, 1)
    s, k = torch.cat((-(w0 + wl), -w0, w1, w1 + wu), 2), torch.cat((lo, c, hi), 2)
    return tuple(None if t is None else t.to(dtype) for t in qp[:6] + (s, k))


# the steps the rows must be far from: l1eq has no outer kinks and bandeq IS the band
TERM = TT.Table(name="pwl", weights=1, aux="piece", grads=GRADS8, term=PwlTerm,
                others={"plain": (PwlPlain, ()), "band": (PwlAsBand, ("l1eq", "bandeq"))}, far_keys=("z",), data=pwl_data,
                stop_inputs=stop_inputs, label=lambda sol: sol["piece"].double(), what="piece", grad_recipe=grad_recipe,
                recipe_data=(1,), tables={"ROWS": ROWS, "GRAD_ROWS": GRAD_ROWS}, share=SHARE, empty=EMPTY, pooled_below=129)
solve_pwl, pwl_inputs, truth = TERM.solve, TERM.inputs, TERM.truth
row_truth, truth_grads, stop_truth = TERM.row_truth, TERM.truth_grads, TERM.stop_truth
cot_of, excused = TT.cot_of, TT.excused
