"""The cases of control['alpha'], the over-relaxed ADMM step, and their truth (no GPU needed to import this module).
tests/test_relax_table.py checks them on the CPU, tests/test_gpu_relax.py runs them.

The truth is `solve_relaxed`: ``oracle.solve_box_qp`` itself, the one loop the reference-made goldens pin, with its ``alpha``
argument -- the relaxed step

    xh = alpha x + (1 - alpha) z_prev;  z = clamp(xh + u);  r = x - z;  s = rho (z - z_prev);  u = u + (xh - z)

At alpha = 1 the argument changes no bit (test_relax_table.py).  Everything else of an iteration -- right-hand side, the six norms of
a check with x_inf taken from x, the rho events, the returned x -- does not know about alpha.

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
    """``oracle.solve_box_qp`` with the over-relaxed step (its ``alpha`` argument); returns the same dict.  trace: the oracle's."""
    return O.solve_box_qp(Q, p, A, b, lb, ub, control, trace=trace, bounds=bounds, alpha=alpha)


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
    return [solve_relaxed(*E.alone(qp, i), E.control(row), alpha=alpha, **E.ALONE) for i in range(row["B"])]
