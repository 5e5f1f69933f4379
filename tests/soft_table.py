"""The cases of the soft-band layer -- min 0.5 x'Qx + p'x + sum_i [wl_i (lo_i - x_i)_+ + wu_i (x_i - hi_i)_+] over {Ax = b, lb <= x <= ub}
-- and their truth (no GPU needed to import this module).  tests/test_soft_table.py checks them on the CPU, tests/test_gpu_soft.py
runs them.

The truth is `solve_soft`: the oracle's own iteration (``oracle.solve_box_qp``) with `SoftTerm` as its ``term=`` -- the one other
z-update -- through the record `TERM` (tests/term_table.py), exactly as ``l1_table.solve_l1`` is.  In the scaled space of the loop (x = D xs) the data are
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
import math

import torch

from oracle import boxqp_oracle as O
import l1_table as LT
import term_table as TT
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


def prox(v, tl, tu, los, his):
    """S of the step, in exactly its branch form"""
    dh, dl = v - his, v - los
    return torch.where(dh > tu, v - tu, torch.where(dl < -tl, v + tl, torch.minimum(torch.maximum(v, los), his)))


class SoftTerm:
    """wl (lo - x)+ + wu (x - hi)+ for oracle.solve_box_qp(term=): wls = D wl, wus = D wu, los = lo / D, his = hi / D"""

    def __init__(self, wl, wu, lo, hi):
        self.wl, self.wu, self.lo, self.hi = wl, wu, lo, hi

    def scale(self, D):
        self.wls, self.wus, self.los, self.his = D * self.wl, D * self.wu, self.lo / D, self.hi / D

    def step(self, v, rho):
        return prox(v, self.wls / rho, self.wus / rho, self.los, self.his)

    def finish(self, z, u, rho, lbs, ubs, D):
        """the step once more at the returned iterate, in the scaled space (z == his / los by assignment on a kink)"""
        los, his = self.los, self.his
        v = z + u
        tl, tu = self.wls / rho + torch.zeros_like(v), self.wus / rho + torch.zeros_like(v)
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
        return {"zone": zone, "u_box": u_box, "margin": margin}


class SoftPlain(SoftTerm):
    """the iterate of a kernel that ignores the band (the classification behind the loop is the band's all the same)"""

    def step(self, v, rho):
        return v


class SoftAsL1(SoftTerm):
    """the iterate of a kernel that takes the band for an L1 term around its middle"""

    def scale(self, D):
        super().scale(D)
        self.l1w, self.l1c = D * ((self.wl + self.wu) / 2), ((self.lo + self.hi) / 2) / D

    def step(self, v, rho):
        return LT.shrink(v, self.l1w / rho, self.l1c)


def sets(sol):
    """-> {"z-2", "z-1", "z0", "z1", "z2": the five zones, unclamped; "clamped"}: bool (B, n, 1) each, a partition"""
    clamped = sol["u_box"] != 0
    out = {f"z{k}": (sol["zone"] == k) & ~clamped for k in ZONES}
    out["clamped"] = clamped
    return out


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


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = LT.stop_inputs(torch.float64)
    wl, c = qp[6], qp[7]
    g = torch.Generator().manual_seed(seed + 23)
    lo = c - BAND * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    hi = c + BAND * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    wu = LT.W_RANGE[0] + (LT.W_RANGE[1] - LT.W_RANGE[0]) * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    return tuple(None if t is None else t.to(dtype) for t in qp[:6] + (wl, wu, lo, hi))


# the steps the rows must be far from: l1eq IS the L1 iterate and onesided has no middle
TERM = TT.Table(name="soft", weights=2, aux="zone", grads=GRADS10, term=SoftTerm,
                others={"plain": (SoftPlain, ()), "l1": (SoftAsL1, ("l1eq", "onesided"))}, far_keys=("z",), data=soft_data,
                stop_inputs=stop_inputs, label=lambda sol: sol["zone"].double(), what="zone", grad_recipe=grad_recipe,
                recipe_data=(2, 3), tables={"ROWS": ROWS, "GRAD_ROWS": GRAD_ROWS}, share=SHARE, empty=EMPTY, pooled_below=129)
solve_soft, soft_inputs, truth = TERM.solve, TERM.inputs, TERM.truth
row_truth, truth_grads, stop_truth = TERM.row_truth, TERM.truth_grads, TERM.stop_truth
cot_of, excused = TT.cot_of, TT.excused
