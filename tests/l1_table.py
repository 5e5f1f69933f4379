"""The cases of the L1 layer -- min 0.5 x'Qx + p'x + sum_i w_i |x_i - c_i| over {Ax = b, lb <= x <= ub} -- and their truth (no GPU
needed to import this module).  tests/test_l1_table.py checks them on the CPU, tests/test_gpu_l1.py runs them.

The truth is `solve_l1`: the oracle's own iteration (``oracle.solve_box_qp``, the loop the reference-made goldens pin) with `L1Term`
as its ``term=`` -- the one other z-update -- through the record `TERM` (tests/term_table.py).  In the scaled space of the loop
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
import torch

from oracle import boxqp_oracle as O
import term_table as TT
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

STOP, STOP_CONTROL, STOP_ROW = TT.STOP, TT.STOP_CONTROL, TT.STOP_ROW


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


def shrink(v, t, cs):
    """S of the step, in exactly its branch form"""
    d = v - cs
    return torch.where(d > t, v - t, torch.where(d < -t, v + t, cs + torch.zeros_like(v)))


class L1Term:
    """w'|x - c| for oracle.solve_box_qp(term=): ws = D w, cs = c / D, t = ws / rho"""

    def __init__(self, w, c):
        self.w, self.c = w, c

    def scale(self, D):
        self.ws, self.cs = D * self.w, self.c / D

    def step(self, v, rho):
        return shrink(v, self.ws / rho, self.cs)

    def finish(self, z, u, rho, lbs, ubs, D):
        """the step once more at the returned iterate, in the scaled space (z == cs by assignment on the kink)"""
        cs = self.cs
        v = z + u
        t = self.ws / rho + torch.zeros_like(v)
        d = v - cs
        kink = (t > 0) & ~(d > t) & ~(d < -t)
        side = torch.where(kink, torch.zeros_like(v), torch.where(d < 0, -torch.ones_like(v), torch.ones_like(v)))
        S = shrink(v, t, cs)
        u_box = (S - torch.minimum(torch.maximum(S, lbs), ubs)) / D      # (S - z with the clamp taken again: exactly zero off the bounds)
        # "margin": how far every element is from changing its set -- | |d| - t | and the distance from S to the nearer bound, unscaled
        margin = torch.minimum((d.abs() - t).abs() * D, ((S - lbs).abs().minimum((S - ubs).abs())) * D)
        return {"side": side, "u_box": u_box, "margin": margin}


def sets(sol):
    """-> (kink, thresholded free, clamped): bool (B, n, 1) each, a partition"""
    kink = sol["side"] == 0
    clamped = ~kink & (sol["u_box"] != 0)
    return kink, ~kink & ~clamped, clamped


def grad_recipe(cot, sol, Q, A, lb, ub, c):
    """The eight gradients of `cot` at the solution `sol` of solve_l1: the effective box into the oracle's fixed-point backward"""
    K = sol["side"] == 0
    lb_e, ub_e = torch.where(K, c, lb), torch.where(K, c, ub)
    u_e = torch.where(K, sol["u"], sol["u_box"])
    y = sol["rho"] * u_e
    lams_e = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    dQ, dp, dA, db, dlb_e, dub_e, _ = O.solve_box_qp_grad(cot, sol["x"], u_e, lams_e, sol["nus"], Q, A, lb_e, ub_e, sol["rho"])
    zero = torch.zeros_like(dp)
    return dict(dQ=dQ, dp=dp, dA=dA, db=db, dlb=torch.where(K, zero, dlb_e), dub=torch.where(K, zero, dub_e),
                dw=sol["side"] * dp, dc=torch.where(K, dlb_e + dub_e, zero))


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = O.create_qp_data(n, B, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 11)
    w = W_RANGE[0] + (W_RANGE[1] - W_RANGE[0]) * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    c = torch.minimum(torch.maximum(C_DEV * torch.randn(B, n, 1, generator=g, dtype=torch.float64), qp[4]), qp[5])
    return tuple(None if t is None else t.to(dtype) for t in qp + (w, c))


# (the step that ignores w is the term at w = 0)
TERM = TT.Table(name="l1", weights=1, aux="side", grads=GRADS8, term=L1Term,
                others={"plain": (lambda w, c: L1Term(torch.zeros_like(w), c), ())}, far_keys=("x", "z", "u"), data=l1_data,
                stop_inputs=stop_inputs, label=lambda sol: sol["side"].double(), what="side", grad_recipe=grad_recipe,
                recipe_data=(1,), tables={"ROWS": ROWS, "GRAD_ROWS": GRAD_ROWS})
solve_l1, l1_inputs, truth = TERM.solve, TERM.inputs, TERM.truth
row_truth, truth_grads, stop_truth = TERM.row_truth, TERM.truth_grads, TERM.stop_truth
cot_of, excused = TT.cot_of, TT.excused
