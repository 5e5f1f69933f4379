"""The cases of the Huber layer -- min 0.5 x'Qx + p'x + sum_i w_i H_{delta_i}(x_i - c_i) over {Ax = b, lb <= x <= ub}, with
H_delta(d) = 0.5 d^2 for |d| <= delta and delta |d| - 0.5 delta^2 beyond -- and their truth (no GPU needed to import this module).
tests/test_huber_table.py checks them on the CPU, tests/test_gpu_huber.py runs them.

The truth is `solve_huber`: the oracle's own iteration (``oracle.solve_box_qp``) with `HuberTerm` as its ``term=`` -- the one other
z-update -- through the record `TERM` (tests/term_table.py), exactly as the other four tables' are.  In the scaled space of the loop
(x = D xs) the data are ws = D (D w), cs = c / D, ds = delta / D, and with v = xh + u, d = v - cs, t = ws / rho (a true division, the
rho of this iteration), q = t ds, lim = ds + q, sh = t / (1 + t)

    S = v if t == 0,  v - q if d > lim,  v + q if d < -lim,  v - sh d otherwise;     z = min(max(S, lbs), ubs)

-- these comparisons in this order: the t == 0 branch first (delta = +inf, lim = q = +inf and the quadratic branch always, makes
q = 0 * inf a NaN at t == 0); delta = 0 is no term.  r, s, u, the six norms of a check and the rho events are the oracle's lines.
With w = 0 it returns the oracle's x, z, u, rho, iter bit for bit (test_huber_table.py).  Behind the loop the step's comparisons are
taken once more at the returned iterate (v = z + u): zone = +1 if d > lim, -1 if d < -lim, 0 otherwise and wherever t == 0;
u_box = (u - t clip(z - cs, -ds, ds)) / D where S != clamp(S), exactly 0 elsewhere (the term's own force acts on a clamped element
too, as the log barrier's does); lams is built from u_box.

`grad_recipe` is the backward: the term is C1, so it has no kink sets -- the oracle's ``solve_box_qp_grad`` on Q + diag(curv) with
u_e = u_box, lams_e from u_e and the true box, curv = w where zone == 0, w > 0 and u_box == 0, else 0; then
dw = dp clip(z - c, -delta, delta), dc = -w dp on zone 0 (else 0) and ddelta = w zone dp.

The pinned rows are l1_table's tier rows (``tier_table`` records, the same K, alpha and signatures) with the term's data on top,
and four kinds more: w = 0 on half the elements, delta = +inf on every third element, delta = 0 on every third element, every hard
bound infinite.

The data.  c is l1_table's: normal with deviation C_DEV around zero, where the generator's unconstrained iterates scatter, kept
inside the box; w is uniform in W_RANGE with every fourth element's w = 0 (kind "halfw": every second), delta uniform in DELTA_RANGE.
W_RANGE, DELTA_RANGE, C_DEV and, per row, the seed offset `j` are the first (j = 0, 1, 2, ...) at which, on
the CPU, all of this holds (test_huber_table.py holds every row to it):
  * every sampled problem holds SHARE of its elements in each of the sets quadratic-free, lower-linear-free, upper-linear-free,
    w = 0 (free) and clamped -- but the sets a kind empties by construction, and below n = 129 the share is asked of the row's sampled
    problems together;
  * the float32 truth's zones differ from the float64 truth's on at most 1 % of a problem's elements and only inside the margin;
  * on the gradient rows no sampled element lies within the bar for z of a zone boundary (curv jumps there), and zones and
    clamped set are the same in float32 and float64;
  * the iterates of three other steps miss the row's bar for z by at least 100 x: the plain step, the pure quadratic step (delta =
    inf: a kernel that lost the linear branches) and the L1 step at weight w delta (a kernel that lost the quadratic branch).
What the search found is recorded beside the constants below.
"""
import math

import torch

from oracle import boxqp_oracle as O
import l1_table as LT
import term_table as TT
import tier_table as T

K_FAR, K_NEAR, K_EVENT = LT.K_FAR, LT.K_NEAR, LT.K_EVENT
# (the first candidate tried: weights of the order of Q's diagonal, zones narrower than the spread of c.  What the search found with
#  it stands above J below)
W_RANGE = (0.5, 3.0)          # the weights of the term's elements, uniform
DELTA_RANGE = (0.05, 0.4)     # the widths of the quadratic zone, uniform
C_DEV = LT.C_DEV              # the spread of c around zero, the centre of the generator's unconstrained iterates
SHARE = 0.05                  # every set of every sampled problem holds at least this share of the elements

TIERS = [(name, what.replace("FormL1", "FormHuber").replace("L1 instance", "Huber instance")) for name, what in LT.TIERS]
EVENT_ROW = LT.EVENT_ROW


def _row(name, K, what, kind="plain", alpha=1.0, j=0):
    """j: the seed offset (tier_table.seed_of) the search of the module's docstring found"""
    return dict(LT._row(name, K, what, alpha=alpha, j=j), huber=kind, l1="allinf" if kind == "allinf" else "plain")


# (row key -> j: what the search found; a row that is absent passed at j = 0.  With W_RANGE, DELTA_RANGE and C_DEV as they stand --
#  the first candidate -- every row, the two gradient rows included, passed at j = 0: over all rows the smallest set of a sampled
#  problem held 0.073 of its elements at n >= 129 (0.137 pooled at n = 31), no label of a float32 truth differed from the float64
#  truth's, the other steps missed the bar for z by 1 799 x (the event row, the pure quadratic step) to 7e8 x, and the nearest zone
#  boundary of a gradient row lay 7.0e-5 from its element against a bar for z of 9.2e-6 (float32) and 1.9e-3 against 5.2e-9 (float64).
#  At the event row's own j, below: the smallest set holds 0.064 and the other steps miss the bar by 163 x (L1) to 175 x.)
# The event row asks one thing more of its j, as in log_table.py: behind the event every output hangs on the adapted rho, and the bar
# is R = 4 times ONE float32 realisation's distance from the float64 truth.  Six float32 solves on the CPU -- the inputs as they are,
# and five times with every entry of Q (kept symmetric) and p moved to a neighbouring float at random -- were apart by the factor
# below in their worst output (largest distance over smallest, the worst of x, z, u, lams, nus, rho, u_box; no GPU figure involved):
#   j      0    1     2    3     4    5     6     7    8    9     10    11
#   worst  3.2  14.8  3.2  47.6  1.5  12.0  17.0  9.9  2.0  23.9  21.9  12.9
# j = 4 is the first at which the six agree within a factor of three in every output (log_table.py's rule); its smallest set holds
# 0.064 and every realisation factors twice.
J = {f"{LT.EVENT_ROW}-K{LT.K_EVENT}": 4}

ROWS = {}
for _name, _what in TIERS:
    for _K in (K_FAR, K_NEAR):
        ROWS[f"{_name}-K{_K}"] = _row(_name, _K, _what, alpha=LT.ALPHA if _name in LT.RELAXED else 1.0, j=J.get(f"{_name}-K{_K}", 0))
ROWS[f"{EVENT_ROW}-K{K_EVENT}"] = _row(EVENT_ROW, K_EVENT, "hot / tail forms of the split loop around an adaptive-rho event: q, lim, sh change with rho",
                                       j=J.get(f"{EVENT_ROW}-K{K_EVENT}", 0))
# above 1024 rows a thread of the streaming body owns a second element: its q, lim, sh come back from the workspace
ROWS["wide_n1025_f32-K10"] = _row("wide_n1025_f32", K_FAR, "k_admm_loop<.., FormHuber>, LU branch, n > 1024: the q / lim / sh regions of the workspace are read",
                                  j=J.get("wide_n1025_f32-K10", 0))
ROWS["halfw_n330-K60"] = _row("loop_split0_n330", K_NEAR, "w = 0 on half the elements", kind="halfw", j=J.get("halfw_n330-K60", 0))
ROWS["infdelta_n330-K60"] = _row("loop_split0_n330", K_NEAR, "delta = +inf on every third element: the quadratic branch always", kind="infdelta",
                                 j=J.get("infdelta_n330-K60", 0))
ROWS["zerodelta_n31-K60"] = _row("small_n31_m1", K_NEAR, "delta = 0 on every third element: no term there", kind="zerodelta",
                                 j=J.get("zerodelta_n31-K60", 0))
ROWS["allinf_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "every hard bound infinite: the loop schedule all the same", kind="allinf",
                               j=J.get("allinf_n129-K60", 0))

SAME_BITS = LT.SAME_BITS
GRAD_ROWS = {"sweep2_n129_m1": _row("sweep2_n129_m1", K_NEAR, "gradients, split loop", j=J.get("grad:sweep2_n129_m1", 0)),
             "lu1_n300_f64": _row("lu1_n300_f64", K_NEAR, "gradients, streaming LU float64", j=J.get("grad:lu1_n300_f64", 0))}
GRADS9 = ("dQ", "dp", "dA", "db", "dlb", "dub", "dw", "dc", "ddelta")
OUTPUTS = T.OUTPUTS + ("zone", "u_box")
SETS = ("quad_free", "lower_free", "upper_free", "zero_free", "clamped")
# the sets a kind empties by construction (the share is not asked of them)
EMPTY = {"allinf": ("clamped",)}

STOP, STOP_CONTROL, STOP_ROW = TT.STOP, TT.STOP_CONTROL, TT.STOP_ROW


def huber_data(r, i, lb, ub):
    """(w, c, delta) of problem i of row r, float64 (n, 1)"""
    n = r["n"]
    kind = r.get("huber", "plain")
    g = torch.Generator().manual_seed(T.seed_of(r) * 49979687 + 19 * i + 11)
    w = W_RANGE[0] + (W_RANGE[1] - W_RANGE[0]) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    c = C_DEV * torch.randn(n, 1, generator=g, dtype=torch.float64)
    c = torch.minimum(torch.maximum(c, lb), ub)          # (the centre stays inside the box)
    delta = DELTA_RANGE[0] + (DELTA_RANGE[1] - DELTA_RANGE[0]) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    if kind == "halfw":
        w[0::2] = 0.0
    else:
        w[0::4] = 0.0
    if kind == "infdelta":
        delta[1::3] = math.inf
    if kind == "zerodelta":
        delta[1::3] = 0.0
    return w, c, delta


def prox(v, t, cs, ds):
    """S of the step, in exactly its branch form (q, lim, sh as the kernels keep them per launch)"""
    on = t != 0
    one = torch.ones_like(v)
    ts = torch.where(on, t + 0 * v, one)                 # (the products with an infinite delta are taken on their own branch only)
    q = ts * ds
    lim = ds + q
    sh = ts / (1 + ts)
    d = v - cs
    return torch.where(~on, v, torch.where(d > lim, v - q, torch.where(d < -lim, v + q, v - sh * d)))


class HuberTerm:
    """w' H_delta(x - c) for oracle.solve_box_qp(term=): ws = D (D w), cs = c / D, ds = delta / D, t = ws / rho"""

    def __init__(self, w, c, delta):
        self.w, self.c, self.delta = w, c, delta

    def scale(self, D):
        self.ws, self.cs, self.ds = D * (D * self.w), self.c / D, self.delta / D

    def step(self, v, rho):
        return prox(v, self.ws / rho, self.cs, self.ds)

    def finish(self, z, u, rho, lbs, ubs, D):
        """the step's comparisons once more at the returned iterate, in the scaled space"""
        cs, ds = self.cs, self.ds
        v = z + u
        t = self.ws / rho + torch.zeros_like(v)
        on = t != 0
        one, zero, inf = torch.ones_like(v), torch.zeros_like(v), torch.full_like(v, math.inf)
        ts = torch.where(on, t, one)
        lim = ds + ts * ds
        d = v - cs
        zone = torch.where(~on, zero, torch.where(d > lim, one, torch.where(d < -lim, -one, zero)))
        S = self.step(v, rho)
        held = S != torch.minimum(torch.maximum(S, lbs), ubs)
        force = ts * torch.minimum(torch.maximum(z - cs, -ds), ds)
        u_box = torch.where(held, torch.where(on, u - force, u) / D, zero)
        # "margin": how far every element is from changing its set -- the distance from |d| to lim (none where t == 0, infinite at an
        # infinite delta) and from S to the nearer bound, unscaled; "zmargin": the first of the two alone, where curv jumps
        zmargin = torch.where(on, (d.abs() - lim).abs(), inf) * D
        margin = torch.minimum(zmargin, (S - lbs).abs().minimum((S - ubs).abs()) * D)
        return {"zone": zone, "u_box": u_box, "margin": margin, "zmargin": zmargin}


class HuberPlain(HuberTerm):
    """the iterate of a kernel that ignores the term (the classification behind the loop is the term's all the same)"""

    def step(self, v, rho):
        return v


class HuberQuadratic(HuberTerm):
    """the iterate of a kernel that lost the linear branches: delta = +inf"""

    def step(self, v, rho):
        return prox(v, self.ws / rho, self.cs, torch.full_like(self.ds, math.inf))


class HuberAsL1(HuberTerm):
    """the iterate of a kernel that lost the quadratic branch: the L1 step at weight w delta (no step at all where that is not a
    weight: w = 0, or an infinite delta)"""

    def step(self, v, rho):
        t = self.ws / rho + torch.zeros_like(v)
        ok = (t != 0) & torch.isfinite(self.ds + torch.zeros_like(v))
        q = torch.where(ok, t, torch.zeros_like(v)) * torch.where(ok, self.ds + torch.zeros_like(v), torch.zeros_like(v))
        return torch.where(ok, LT.shrink(v, q, self.cs), v)


def sets(sol, w):
    """-> {quad_free, lower_free, upper_free, zero_free, clamped}: bool (B, n, 1) each, a partition"""
    clamped, on, zone = sol["u_box"] != 0, w > 0, sol["zone"]
    return {"quad_free": on & ~clamped & (zone == 0), "lower_free": on & ~clamped & (zone == -1), "upper_free": on & ~clamped & (zone == 1),
            "zero_free": ~on & ~clamped, "clamped": clamped}


def curv_of(sol, w):
    """the diagonal the backward adds on the free set: w on the free elements of the quadratic zone"""
    return torch.where((sol["zone"] == 0) & (w > 0) & (sol["u_box"] == 0), w, torch.zeros_like(w))


def grad_recipe(cot, sol, Q, A, lb, ub, w, c, delta):
    """The nine gradients of `cot` at the solution `sol` of solve_huber: the oracle's fixed-point backward on Q + diag(curv)"""
    u_e = sol["u_box"]
    y = sol["rho"] * u_e
    lams_e = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    Qc = Q + torch.diag_embed(curv_of(sol, w)[:, :, 0])
    dQ, dp, dA, db, dlb, dub, _ = O.solve_box_qp_grad(cot, sol["x"], u_e, lams_e, sol["nus"], Qc, A, lb, ub, sol["rho"])
    zone, zero = sol["zone"].to(dp.dtype), torch.zeros_like(dp)
    return dict(dQ=dQ, dp=dp, dA=dA, db=db, dlb=dlb, dub=dub, dw=dp * torch.minimum(torch.maximum(sol["z"] - c, -delta), delta),
                dc=torch.where(zone == 0, -w * dp, zero), ddelta=w * zone * dp)


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = O.create_qp_data(n, B, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 37)
    w = W_RANGE[0] + (W_RANGE[1] - W_RANGE[0]) * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    w[:, 0::4] = 0.0
    c = torch.minimum(torch.maximum(C_DEV * torch.randn(B, n, 1, generator=g, dtype=torch.float64), qp[4]), qp[5])
    delta = DELTA_RANGE[0] + (DELTA_RANGE[1] - DELTA_RANGE[0]) * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    return tuple(None if t is None else t.to(dtype) for t in qp + (w, c, delta))


TERM = TT.Table(name="huber", weights=1, aux="zone", grads=GRADS9, term=HuberTerm,
                others={"plain": (HuberPlain, ()), "quadratic": (HuberQuadratic, ()), "l1": (HuberAsL1, ())}, far_keys=("z",),
                data=huber_data, stop_inputs=stop_inputs, label=lambda sol: sol["zone"].double(), what="zone", grad_recipe=grad_recipe,
                recipe_data=(0, 1, 2), tables={"ROWS": ROWS, "GRAD_ROWS": GRAD_ROWS}, share=SHARE, empty=EMPTY, pooled_below=129)
solve_huber, huber_inputs, truth = TERM.solve, TERM.inputs, TERM.truth
row_truth, truth_grads, stop_truth = TERM.row_truth, TERM.truth_grads, TERM.stop_truth
cot_of, excused = TT.cot_of, TT.excused
