"""The cases of control['stop'] = 'each' (tests/test_each_table.py checks them on the CPU, tests/test_gpu_each.py runs them).

The truth for problem b of a row is the oracle's solve of the slice [b:b+1] of every input -- the reference's algorithm on a batch
of one -- with the bound flags of the WHOLE batch passed through ``bounds=`` (any_lb / any_ub stay global).

A row draws its problems from the oracle's generator (``create_qp_data``; ``hard``: ``create_hard_qp_data``) and makes them
heterogeneous: problem b gets p * s_b (and b * s_b), with s_b spread evenly in the logarithm over ``p_decades`` decades, and a box
[lb, ub] * w_b with w_b spread the same way over ``w_decades``.  Every problem keeps finite bounds on both sides.  Rows through an
adaptive-rho event use the recipe that fires at iteration 100: Q * 50, rho = 100., scale = False, adaptive_rho = True.

``iters`` is what the float32 AND the float64 oracle give for every problem (the seeds were tried until they agree on all of
them: a problem whose stop verdict hangs on rounding would make the GPU comparison a coin toss); ``adapts`` likewise which problems
change rho at the event.  test_each_table.py recomputes both.
"""
import functools

import torch

from oracle import boxqp_oracle as O

EVENT = dict(rho=100., scale=False, adaptive_rho=True)      # (with Q * 50: `q_scale`)

ROWS = {}


def _row(name, **kw):
    kw.setdefault("m", 1)
    kw.setdefault("hard", False)
    kw.setdefault("q_scale", 1.0)
    kw.setdefault("p_decades", 2.0)
    kw.setdefault("w_decades", 0.5)
    kw.setdefault("w_top", 0.0)
    kw.setdefault("b_with_p", False)
    kw.setdefault("infeasible_last", False)
    kw.setdefault("adapts", None)
    kw.setdefault("never", [])
    ROWS[name] = dict(kw, name=name)


def spread(B, decades, top=0.0):
    """B factors, evenly spaced in the logarithm, from 10^-decades to 10^top"""
    if B == 1:
        return torch.ones(1, dtype=torch.float64)
    return 10.0 ** (-decades + (decades + top) * torch.arange(B, dtype=torch.float64) / (B - 1))


def inputs(row, dtype=torch.float64):
    """-> Q, p, A, b, lb, ub of the row in `dtype` (drawn once in float64 and rounded: both dtypes see the same problems)"""
    n, B, m, seed = row["n"], row["B"], row["m"], row["seed"]
    if row["hard"]:
        Q, p, A, b, lb, ub = O.create_hard_qp_data(n, 0.15, [seed + i for i in range(B)], dtype=torch.float64)
        # the hard generator centres its box on a random point: scale the box about that centre
        mid, half = (lb + ub) / 2, (ub - lb) / 2
        half = half * spread(B, row["w_decades"], row["w_top"]).view(B, 1, 1)
        lb, ub = mid - half, mid + half
        if m == 0:
            A = b = None
        else:
            A, b = A[:, :m].contiguous(), b[:, :m].contiguous()
    else:
        Q, p, A, b, lb, ub = O.create_qp_data(n, B, seed=seed, with_eq=m > 0, dtype=torch.float64)
        w = spread(B, row["w_decades"], row["w_top"]).view(B, 1, 1)
        lb, ub = lb * w, ub * w
        if m > 1:
            # more equality rows than the generator's one: random rows through a point well inside every box
            g = torch.Generator().manual_seed(seed + 1000)
            A = torch.cat((A, torch.randn(B, m - 1, n, generator=g, dtype=torch.float64)), 1)
            x0 = (torch.rand(B, n, 1, generator=g, dtype=torch.float64) - 0.5) * w
            b = torch.matmul(A, x0)
        elif m == 1:
            b = b * w
    Q = Q * row["q_scale"]
    s_b = spread(B, row["p_decades"]).flip(0).view(B, 1, 1)
    p = p * s_b
    if row["b_with_p"] and b is not None:       # (the right-hand side shrinks with p: x = 0 is then nearly optimal for the smallest)
        b = b * s_b
    if row["infeasible_last"]:                  # (the last problem's equality row cannot be met inside its box: it never becomes optimal)
        b[-1] = 10.0 * ub[-1].abs().sum()
    cast = lambda t: None if t is None else t.to(dtype).contiguous()
    return tuple(cast(t) for t in (Q, p, A, b, lb, ub))


def control(row, **extra):
    return O.make_control(**dict(row["control"], **extra))


ALONE = dict(bounds=(True, True))      # the bound flags of the whole batch, for a problem solved on its own: every table's are both finite


def alone(qp, i):
    """-> problem i of the inputs `qp` as a batch of one (to be solved with **ALONE)"""
    return tuple(None if t is None else t[i:i + 1] for t in qp)


@functools.lru_cache(maxsize=None)
def solo(name, dtype):
    """-> the oracle's solution of every problem of the row on its own: a list of B dicts (plus "n_factor"), computed once"""
    row = ROWS[name]
    qp = inputs(row, dtype)
    out = []
    for i in range(row["B"]):
        trace = {}
        sol = O.solve_box_qp(*alone(qp, i), control(row), trace=trace, **ALONE)
        sol["n_factor"] = trace["n_factor"]
        out.append(sol)
    return out


def solo_iters(name, dtype):
    return [int(s["iter"]) for s in solo(name, dtype)]


def solo_adapts(name, dtype):
    return [s["n_factor"] > 1 for s in solo(name, dtype)]


# every row: per-problem scales of p (and of b with it) over several decades -- the smallest problems are optimal at the first or
# second check, the largest run five to ten times as long
PLAIN = dict(eps_abs=1e-4, eps_rel=1e-4, max_iters=1500, adaptive_rho=False)
THROUGH_EVENT = dict(eps_abs=1e-4, eps_rel=1e-4, max_iters=1500, **EVENT)

_row("small_n100", n=100, B=8, m=0, seed=1, p_decades=5., b_with_p=True, control=PLAIN, dtype=torch.float32,
     iters=[20, 60, 60, 50, 30, 10, 10, 0])
_row("small_n50_event", n=50, B=8, m=1, seed=1, q_scale=50., p_decades=6., b_with_p=True, control=THROUGH_EVENT, dtype=torch.float32,
     iters=[100, 90, 100, 50, 20, 10, 0, 0], adapts=[True, False, True, False, False, False, False, False])
_row("split_n130", n=130, B=8, m=1, seed=1, p_decades=5., b_with_p=True, control=PLAIN, dtype=torch.float32,
     iters=[20, 50, 50, 40, 30, 10, 0, 0])
_row("split_n449", n=449, B=8, m=1, seed=1, p_decades=5., b_with_p=True, control=PLAIN, dtype=torch.float32,
     iters=[20, 60, 80, 60, 40, 20, 20, 0])
_row("split_n130_event", n=130, B=8, m=1, seed=1, q_scale=50., p_decades=6., b_with_p=True, control=THROUGH_EVENT, dtype=torch.float32,
     iters=[100, 100, 80, 50, 20, 10, 0, 0], adapts=[True, True, False, False, False, False, False, False])
_row("lu_n130_m17", n=130, B=6, m=17, seed=1, p_decades=5., b_with_p=True, control=PLAIN, dtype=torch.float32,
     iters=[30, 50, 40, 20, 10, 0])
_row("f64_n70_m3", n=70, B=8, m=3, seed=1, p_decades=5., b_with_p=True, control=PLAIN, dtype=torch.float64,
     iters=[20, 50, 60, 40, 20, 10, 0, 0])
_row("f64_n70_m3_event", n=70, B=8, m=3, seed=1, q_scale=50., p_decades=6., b_with_p=True, control=THROUGH_EVENT, dtype=torch.float64,
     iters=[100, 100, 90, 50, 20, 10, 10, 0], adapts=[True, True, False, False, False, False, False, False])
# the host-driven persistent schedule, whose chunks end in k_check_done: n <= 25 checks at every iteration, a chunk is 512 iterations.
# A slowly converging solve (a given rho far too small, no scaling): one problem stops behind the first chunk boundary, two never become
# optimal (`never`: the first is too slow for max_iters, the last cannot meet its equality row inside its box) and end at max_iters - 1.
# With a check at EVERY iteration a count is the exact iteration at which a slowly falling residual (about half a percent per
# iteration here) crosses its tolerance, so agreement of the two oracles is not enough: the tolerance is 1e-3, where float32 rounding
# (1e-7 of the scale) is 0.01 % of it, and the seed is one at which every count stays put when the tolerance moves by +-0.2 %, twenty
# times that (test_each_table.py checks it, in both dtypes)
_row("chunk_n20", n=20, B=6, m=1, seed=4, p_decades=4., b_with_p=True, infeasible_last=True,
     control=dict(eps_abs=1e-3, eps_rel=1e-3, max_iters=1200, adaptive_rho=False, rho=0.003, scale=False), dtype=torch.float32,
     iters=[1199, 600, 0, 0, 0, 1199], never=[0, 5])
# above 1024 rows (the gated refactorisation chain): two problems, as few as cross the event (at iteration 90: a check every 30) with
# one that adapts and one that does not -- a batch of two cannot show three distinct counts
_row("big_n1030", n=1030, B=2, m=1, seed=1, q_scale=50., p_decades=4., b_with_p=True, control=dict(THROUGH_EVENT, max_iters=400),
     dtype=torch.float32, iters=[90, 30], adapts=[True, False])
