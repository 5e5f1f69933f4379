"""The cases of the log-barrier layer -- min 0.5 x'Qx + p'x - sum_i w_i log(x_i) over {Ax = b, lb <= x <= ub}, w >= 0 -- and their
truth (no GPU needed to import this module).  tests/test_log_table.py checks them on the CPU, tests/test_gpu_log.py runs them.

The truth is `solve_log`: the oracle's own iteration (``oracle.solve_box_qp``) with `LogTerm` as its ``term=`` -- the one other
z-update -- through the record `TERM` (tests/term_table.py), exactly as ``l1_table.solve_l1`` and ``soft_table.solve_soft`` are.  In
the scaled space of the loop (x = D xs) the barrier is -w_i log(xs_i) plus a constant, so ws = w (the equilibration scales Q, p by D and the equality rows by
E; the objective has no scalar scale).  With v = xh + u, t = ws / rho (a true division, the rho of this iteration) and
s = sqrt(v v + 4 t)

    S = v if t == 0,  0.5 (v + s) if v >= 0,  2 t / (s - v) if v < 0;     z = min(max(S, lbs), ubs)

r, s, u, the six norms of a check and the rho events are the oracle's lines.  With w = 0 it returns the oracle's x, z, u, rho, iter
bit for bit (test_log_table.py).  Behind the loop the step is evaluated once more at the returned iterate (v = z + u):
u_box = (u + t / z) / D where S != clamp(S), exactly 0 elsewhere; curv = w / z^2 (unscaled z) where w > 0 and u_box == 0, else 0;
lams is built from u_box.

`grad_recipe` is the backward: the oracle's ``solve_box_qp_grad`` on Q + diag(curv) with u_e = u_box, lams_e from u_e and the true
box, then dw = -dp / z where w > 0, else 0.

The pinned rows are l1_table's tier rows (``tier_table`` records, the same K, alpha and signatures) with the barrier's weights on
top, and four kinds more: zero weights on half the elements, positive lower bounds under barrier elements, weights so small that
the v < 0 branch of the step is taken, every hard bound infinite.

The weights.  W_RANGE and, per row, the seed offset `j` are the first (j = 0, 1, 2, ...) at which, on the CPU, every sampled
problem holds SHARE of its elements in each of the four sets (barrier / w = 0) x (free / clamped) -- but the sets a kind empties by
construction --, the float32 truth's clamped set differs from the float64 truth's on at most 1 % of a problem's elements and only
inside the margin, and the plain step's iterate misses the bar for z by at least 100 x (test_log_table.py holds every row to all
three).  In the plain kind every third element has w = 0; an element whose upper bound is not positive (a few of the tier rows'
lb == ub elements) has w = 0 too: with w > 0 its domain would be empty and the solve refuses it.
"""
import torch

from oracle import boxqp_oracle as O
import l1_table as LT
import term_table as TT
import tier_table as T

K_FAR, K_NEAR, K_EVENT = LT.K_FAR, LT.K_NEAR, LT.K_EVENT
W_RANGE = (0.05, 0.5)         # the budgets of the barrier elements, uniform
W_TINY = (1e-4, 1e-2)         # kind "tiny"
SHARE = 0.05                  # every set of every sampled problem holds at least this share of the elements

TIERS = [(name, what.replace("FormL1", "FormLog").replace("L1 instance", "log instance")) for name, what in LT.TIERS]
EVENT_ROW = LT.EVENT_ROW


def _row(name, K, what, kind="plain", alpha=1.0, j=0):
    """j: the seed offset (tier_table.seed_of) the search of the module's docstring found"""
    return dict(LT._row(name, K, what, alpha=alpha, j=j), log=kind)


# (row key -> j: what the search found.  With W_RANGE and W_TINY as they stand every row, the two gradient rows included, passed at
#  j = 0; the event row asks one thing more of its j)
# The event row's j.  Behind the event every output hangs on the adapted rho, a square root of a ratio of four inf-norms, and the bar
# is R = 4 times ONE float32 realisation's distance from the float64 truth.  With the barrier's step that distance is not a stable
# figure at any seed: six float32 solves on the CPU -- the inputs as they are, and five times with every entry of Q (kept symmetric)
# and p moved to a neighbouring float at random, a relative 2^-24 -- were apart by the factor below in their worst output (largest
# distance over smallest, the worst of x, z, u, lams, nus, rho, u_box; float64 solves on the CPU, no GPU figure involved):
#   j      0    1    2    3    4    5    6    7    8    9    10   11   12   13   14   15   16   17   18   19   20   21   22   23
#   worst  8.4  15.9 3.6  26.5 7.0  13.4 2.9  6.9  3.4  8.9  9.3  78.4 3.7  50.1 6.4  11.2 5.8  24.8 56.2 19.9 15.9 12.8 117  2.9
# (j = 24 .. 47: between 3.3 and 37; at j = 0 nus alone spans 4.4e-6 .. 3.7e-5, and the float32 truth of another CPU fell outside the
# span this one gave at several j.)  j = 6 is the first at which the six agree within a factor of three in every output, the smallest
# set holds SHARE (0.13) and every realisation factors twice.  A bar drawn from one realisation still asks float32 arithmetic to stay
# within 4 / 2.9 of its own scatter: of all rows this one's verdict is the least stable, by what it measures and not by what runs.
J = {f"{LT.EVENT_ROW}-K{LT.K_EVENT}": 6}

ROWS = {}
for _name, _what in TIERS:
    for _K in (K_FAR, K_NEAR):
        ROWS[f"{_name}-K{_K}"] = _row(_name, _K, _what, alpha=LT.ALPHA if _name in LT.RELAXED else 1.0, j=J.get(f"{_name}-K{_K}", 0))
ROWS[f"{EVENT_ROW}-K{K_EVENT}"] = _row(EVENT_ROW, K_EVENT, "hot / tail forms of the split loop around an adaptive-rho event: t changes with rho",
                                       j=J.get(f"{EVENT_ROW}-K{K_EVENT}", 0))
# above 1024 rows a thread of the streaming body owns a second element: its t comes back from the workspace
ROWS["wide_n1025_f32-K10"] = _row("wide_n1025_f32", K_FAR, "k_admm_loop<.., FormLog>, LU branch, n > 1024: the t region of the workspace is read",
                                  j=J.get("wide_n1025_f32-K10", 0))
ROWS["halfw_n330-K60"] = _row("loop_split0_n330", K_NEAR, "w = 0 on half the elements", kind="halfw", j=J.get("halfw_n330-K60", 0))
ROWS["poslb_n31-K60"] = _row("small_n31_m1", K_NEAR, "lb_i > 0 on every fifth barrier element: barrier elements rest on a lower bound", kind="poslb",
                             j=J.get("poslb_n31-K60", 0))
ROWS["tiny_n330-K60"] = _row("loop_split0_n330", K_NEAR, "weights so small that the v < 0 branch of the step is taken", kind="tiny",
                             j=J.get("tiny_n330-K60", 0))
ROWS["allinf_n129-K60"] = _row("sweep2_n129_m1", K_NEAR, "every hard bound infinite: the loop schedule all the same", kind="allinf",
                               j=J.get("allinf_n129-K60", 0))

SAME_BITS = LT.SAME_BITS
GRAD_ROWS = {"sweep2_n129_m1": _row("sweep2_n129_m1", K_NEAR, "gradients, split loop", j=J.get("grad:sweep2_n129_m1", 0)),
             "lu1_n300_f64": _row("lu1_n300_f64", K_NEAR, "gradients, streaming LU float64", j=J.get("grad:lu1_n300_f64", 0))}
GRADS7 = ("dQ", "dp", "dA", "db", "dlb", "dub", "dw")
OUTPUTS = T.OUTPUTS + ("u_box", "curv")
SETS = ("barrier_free", "barrier_clamped", "zero_free", "zero_clamped")
# the sets a kind empties by construction (the share is not asked of them)
EMPTY = {"allinf": ("barrier_clamped", "zero_clamped")}

STOP, STOP_CONTROL, STOP_ROW = LT.STOP, LT.STOP_CONTROL, LT.STOP_ROW


def log_data(r, i, lb, ub):
    """(w, lb) of problem i of row r, float64 (n, 1): the kind "poslb" moves lower bounds, every other kind returns lb as it is"""
    n = r["n"]
    kind = r.get("log", "plain")
    g = torch.Generator().manual_seed(T.seed_of(r) * 32452843 + 13 * i + 5)
    lo, hi = W_TINY if kind == "tiny" else W_RANGE
    w = lo + (hi - lo) * torch.rand(n, 1, generator=g, dtype=torch.float64)
    up = torch.rand(n, 1, generator=g, dtype=torch.float64)
    if kind == "halfw":
        w[0::2] = 0.0
    else:
        w[0::3] = 0.0
    w[~(ub > 0)] = 0.0          # (the domain of a barrier element must not be empty)
    if kind == "poslb":
        lb = lb.clone()
        bar = torch.nonzero(w[:, 0] > 0)[:, 0][0::5]
        lb[bar] = torch.minimum(0.2 + 0.6 * up[bar], ub[bar])
    return w, lb


def prox(v, t):
    """S of the step, in exactly its branch form"""
    s = torch.sqrt(v * v + 4 * t)
    safe = torch.where(v < 0, s - v, torch.ones_like(s))          # (the division is taken on its own branch only)
    return torch.where(t == 0, v, torch.where(v >= 0, 0.5 * (v + s), (2 * t) / safe))


class LogTerm:
    """-w' log x for oracle.solve_box_qp(term=): the barrier is -w_i log(xs_i) plus a constant in the scaled space, so ws = w"""

    def __init__(self, w):
        self.w = w

    def scale(self, D):
        pass

    def step(self, v, rho):
        return prox(v, self.w / rho)

    def finish(self, z, u, rho, lbs, ubs, D):
        """the step once more at the returned iterate, in the scaled space"""
        ws = self.w
        v = z + u
        t = ws / rho + torch.zeros_like(v)
        S = self.step(v, rho)
        held = S != torch.minimum(torch.maximum(S, lbs), ubs)
        zsafe = torch.where(t == 0, torch.ones_like(z), z)
        u_box = torch.where(held, (u + t / zsafe) / D, torch.zeros_like(v))
        zu = D * z
        curv = torch.where((ws > 0) & ~held, ws / (zu * zu), torch.zeros_like(v))
        # "margin": how far every element is from changing its set -- the distance from S to the nearer bound, unscaled
        margin = (S - lbs).abs().minimum((S - ubs).abs()) * D
        return {"u_box": u_box, "curv": curv, "margin": margin}


class LogPlain(LogTerm):
    """the iterate of a kernel that ignores the barrier"""

    def step(self, v, rho):
        return v


def sets(sol, w):
    """-> {barrier_free, barrier_clamped, zero_free, zero_clamped}: bool (B, n, 1) each, a partition"""
    clamped, bar = sol["u_box"] != 0, w > 0
    return {"barrier_free": bar & ~clamped, "barrier_clamped": bar & clamped, "zero_free": ~bar & ~clamped, "zero_clamped": ~bar & clamped}


def grad_recipe(cot, sol, Q, A, lb, ub, w):
    """The seven gradients of `cot` at the solution `sol` of solve_log: the oracle's fixed-point backward on Q + diag(curv)"""
    u_e = sol["u_box"]
    y = sol["rho"] * u_e
    lams_e = torch.cat((torch.relu(-y), torch.relu(y)), 1)
    Qc = Q + torch.diag_embed(sol["curv"][:, :, 0])
    dQ, dp, dA, db, dlb, dub, _ = O.solve_box_qp_grad(cot, sol["x"], u_e, lams_e, sol["nus"], Qc, A, lb, ub, sol["rho"])
    zsafe = torch.where(w > 0, sol["z"], torch.ones_like(dp))
    return dict(dQ=dQ, dp=dp, dA=dA, db=db, dlb=dlb, dub=dub, dw=torch.where(w > 0, -dp / zsafe, torch.zeros_like(dp)))


def stop_inputs(dtype):
    n, B, seed = STOP
    qp = O.create_qp_data(n, B, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(seed + 29)
    w = W_RANGE[0] + (W_RANGE[1] - W_RANGE[0]) * torch.rand(B, n, 1, generator=g, dtype=torch.float64)
    w[:, 0::3] = 0.0
    w[~(qp[5] > 0)] = 0.0
    return tuple(None if t is None else t.to(dtype) for t in qp + (w,))


class LogTable(TT.Table):
    def inputs(self, r, B, idx=None):
        """(Q, p, A, b, lb, ub, w): the lower bounds are log_data's (the kind "poslb" moves them; 0 < lb <= ub stays in float32)"""
        *qp, w, lb = super().inputs(r, B, idx)
        return (*qp[:4], lb, qp[5], w)


TERM = LogTable(name="log", weights=1, aux="curv", grads=GRADS7, term=LogTerm, others={"plain": (LogPlain, ())},
                far_keys=("z",), data=log_data, stop_inputs=stop_inputs, label=lambda sol: sol["u_box"] != 0, what="clamped set",
                grad_recipe=grad_recipe, recipe_data=(0,), tables={"ROWS": ROWS, "GRAD_ROWS": GRAD_ROWS}, share=SHARE, empty=EMPTY)
solve_log, log_inputs, truth = TERM.solve, TERM.inputs, TERM.truth
row_truth, truth_grads, stop_truth = TERM.row_truth, TERM.truth_grads, TERM.stop_truth
cot_of, excused = TT.cot_of, TT.excused
