"""The backward of ``unroll=True`` as data (no GPU needed to import this module): one row per kernel instantiation, size boundary
and knob of the unroll tape (csrc/lqp_unroll.hpp, lqp_boxqp_unroll_* / lqp_unroll_scale_* in csrc/lqp_amd.hip,
lqp_py_amd/unrolled.py).  The machinery is tests/tier_table.py's: `row`, `batch`, `sample`, `seed_of`, `inputs` (lb = -inf, ub = +inf,
lb == ub entries, active and inactive bounds, random A) and the bar `compare`.

The truth of a row is autograd through the CPU oracle's own loop (oracle.boxqp_oracle.unrolled_grad) in float64, pinned to K
iterations; the budget is the same tape in float32.  tests/test_gpu_unroll.py runs every row on the GPU; tests/test_unroll_table.py
checks without one that the rows cover every knob and both sides of every boundary, that every row's clamp decisions are settled
(`settled`), and that the comparator sees a wrong tape.

Row fields on top of tier_table's:
  ctl     also beta (a float, or "tensor": one value per problem), check_solved, adaptive_rho_iter, linsolve
  j       seed offset found by the deterministic seed search (tests/tools/unroll_seed_search.py): the smallest j < 16 for which the
          row's sampled problems meet `settled`; the GPU run does not search
  family  "one" (k_unroll_sweep, n <= 512) | "split" (k_unroll_sweep_split) | "big" (k_unroll_sweep, 512 < n <= 1024) |
          "lu32" | "lu64" (k_unroll_sweep_lu) | "ev32" | "ev64" (lqp_boxqp_unroll_tape_segment / _finish) | "taped" (torch ops)
  exp     what the run must report: `ub`, `us` = launches of the profile classes unroll_backward / unroll_scaling of one backward,
          linsolve_used and n_factor of the forward (from the functional solve under the same control: the unroll forward solves on
          a private workspace)
  split   symmetric float32 rows with 128 < n <= 512: True = the sweep runs on two workgroups per QP, i.e. LQP_UNROLL_SPLIT=0 must
          change gradient bits; False = the one-workgroup sweep runs by itself and LQP_UNROLL_SPLIT=0 must not change a bit
          (both sweeps launch once: the launch counts alone cannot tell them apart)

What the rows found (measured on an MI355X, see each row's `why`):
  * 513 <= n <= 1024 in float32 runs the one-workgroup k_unroll_sweep on the packed inverse of the two-steps-per-pass forward, with
    rl = unroll_lds_blocks(m, Ks) of the blocks LDS-resident and the rest streamed per product: a correct sweep, no fall-back.
  * lb == ub entries: the kernels give the whole clamp gradient to the side the iterate came from (code -1: dlb, +1: dub), the taped
    loop of torch ops splits it evenly when the iterate came from below (torch.minimum on the tie max(w, lb) == ub).  dlb + dub is
    the same on every path; that sum is what the rows compare there.
  * adaptive_rho_iter is rounded to a multiple of check_solved (reference :139-141): 10 at n = 330 (check_solved = 20) rounds to 0 and
    becomes 1, so that EVERY iteration refactorises with the ratio of the last check.  The float32 event rows set check_solved = 10.
"""
import math

import torch

import tier_table as T
from tier_table import R_DEFAULT, F_DEFAULT, R_MAX, F_MAX, K_DEFAULT, K_EVENTS, RHO_LO, RHO_HI, batch, sample, seed_of, inputs, compare, ks

GRADS = ("dQ", "dp", "dA", "db", "dlb", "dub")
KEYS = ("x", "dQ", "dp", "dA", "db", "dlb", "dub", "dlb+dub@tie")
F64_SETTLED = 100 * 1e-9                # float64 rows: every clamp gap is a hundred times the error the row may have
SPD_MAXM = 16
EV32 = dict(check_solved=10, adaptive_rho_iter=10)
K_EV32 = 30


def _segments(K, ar_iter, ar_max=1000):
    """Segments the epoch walk cuts a tape of K + 1 x-updates into (unrolled._tape_segments)."""
    from lqp_py_amd.unrolled import _tape_segments
    return len(_tape_segments(K + 1, True, ar_iter, ar_max))


def expect(r):
    """Launch counts of one backward and the forward's path, from the row (the selection code restated; see `exp`)."""
    fam, m, env, ctl = r["family"], r["m"], r["env"], r["ctl"]
    f32 = r["dtype"] == "f32"
    if fam == "taped":
        ub, us = 0, 0
    elif fam in ("ev32", "ev64"):
        ub = 2 * _segments(r["K"], ctl.get("adaptive_rho_iter", 100)) + (1 if m > 0 else 0) + 1
        us = 0                                                      # (the scaling by autograd: unrolled._backward_with_rho_events)
    else:
        ub = 2 if fam in ("one", "split", "big") else 2 + (1 if m > 0 else 0)
        sn = env.get("LQP_UNROLL_SCALE_NATIVE", "1")
        if not f32 or sn == "0":
            us = 0
        elif ctl.get("scale", True) is False:
            us = 1                                                  # (scale_grad alone: rho from ||Qs||_F)
        elif sn == "2" or ctl.get("beta") == "tensor":
            us = 3                                                  # (colmax, scale_grad, scatter; the n-sized chain by autograd)
        else:
            us = 5
    return dict(ub=ub, us=us, linsolve_used=1 if fam in ("lu32", "lu64") or not f32 or r.get("lu") else 2, n_factor=r["n_factor"])


def urow(name, n, m, B, family, j=0, n_factor=1, split=None, lu=False, **kw):
    r = T.row(name, n, m, B, **kw)
    r.update(j=j, family=family, n_factor=n_factor, split=split, lu=lu)
    r["flip"] = None
    r["exp"] = expect(r)
    return r


LS_LU = dict(linsolve="lu")
R8_TIE = ("R = 8: the budget of dlb + dub on the ties is a maximum over the four lb == ub entries of the two problems only -- one sample "
          "of a float32 error, not a bound (measured ratio 4.6; every other output of the row is below 1.8)")
R8_M16 = ("R = 8: with m = 16 every product is followed by sixteen float32 dot products of length n (the rank-m equality correction) "
          "that the pivoted LU of the KKT matrix in the oracle has no counterpart of, and dp sums 61 such terms (measured ratio 4.3 and "
          "4.7 on dp, below 4 on every other output)")
K10 = ("K = 3: with over 2000 bound entries per iteration no seed below 16 settles every float32 clamp decision at K = 60, 30 or 10 "
       "(smallest ratios 0.02 ... 2.3), and one float64 tape of K = 60 costs 40 s of host time")

ROWS = [
    # ---------------- float32, symmetric x-update: k_unroll_sweep on one workgroup (n <= 256: Ks < 5 is never split) ----------------
    urow("one_n1_m0", 1, 0, 3, "one", K=20, why="K = 20: one variable converges exactly at iteration 25 (tier_table small_n1_m0)"),
    urow("one_n31_m1", 31, 1, 3, "one"),
    urow("one_n64_m2", 64, 2, 2, "one", R=R_MAX, why=R8_TIE),
    urow("one_n65_m0", 65, 0, 3, "one"),
    urow("one_n128_m1", 128, 1, 3, "one", j=1),
    urow("one_n129_m2", 129, 2, 3, "one", split=False),
    urow("one_n200_m16", 200, 16, 2, "one", split=False),
    urow("one_n256_m1", 256, 1, 2, "one", split=False, why="Ks = 4: below the split sweep's Ks >= 5"),
    # ---------------- k_unroll_sweep_split<Ks, MA>: Ks = 5 ... 8 (P.xchg, 2 B rounded up to 16 <= #CUs), ragged and exact n ----------
    urow("split_n257_m1", 257, 1, 3, "split", split=True),
    urow("split_n320_m2", 320, 2, 2, "split", split=True),
    urow("split_n321_m0", 321, 0, 3, "split", j=1, split=True),
    urow("split_n384_m1", 384, 1, 2, "split", split=True),
    urow("split_n385_m2", 385, 2, 3, "split", j=1, split=True),
    urow("split_n448_m16", 448, 16, 2, "split", split=True, R=R_MAX, why=R8_M16),
    urow("split_n449_m0", 449, 0, 3, "split", j=2, split=True, why="Ks = 8, m = 0: k_unroll_sweep_split<8, 1>"),
    urow("split_n511_m1", 511, 1, 2, "split", split=True, why="Ks = 8, m = 1: <8, 1>"),
    urow("split_n512_m2", 512, 2, 3, "split", j=1, split=True, why="Ks = 8, m = 2: <8, SPD_MAXM>"),
    urow("split_n512_m16", 512, 16, 2, "split", split=True, R=R_MAX,
         why="Ks = 8, m = 16: <8, SPD_MAXM> with every accumulator in use.  " + R8_M16),
    # the split sweep is refused when shared_grid(B, 2) = 16 ceil(B / 8) exceeds #CUs x (workgroups per CU: 1 at 512 threads and this LDS)
    urow("split_near_n449_m1", 449, 1, "cus//2", "split", split=True),
    urow("one_far_n449_m1", 449, 1, "cus//2 + 1", "one", split=False,
         why="shared_grid(B, 2) > #CUs: the split sweep is refused, k_unroll_sweep<1> runs"),
    # ---------------- 512 < n <= 1024: k_unroll_sweep at Ks = 9 ... 16, most of the packed inverse streamed per product ----------------
    urow("big_n513_m2", 513, 2, 2, "big"),
    urow("big_n576_m0", 576, 0, 2, "big"),
    urow("big_n700_m1", 700, 1, 2, "big", j=1),
    urow("big_n1000_m1", 1000, 1, 2, "big"),
    urow("big_n1023_m1", 1023, 1, 2, "big", j=4, why="big_n1023_m0 found no settled seed below 16 (ratios 0.03 ... 4.7)"),
    urow("big_n1024_m1", 1024, 1, 2, "big", j=2),
    # ---------------- the control's variants of the scaling chain ----------------
    urow("noscale_n330", 330, 1, 3, "split", j=1, split=True, ctl=dict(scale=False)),
    urow("rho_given_n330", 330, 1, 3, "split", split=True, ctl=dict(rho=0.5)),
    urow("beta_float_n330", 330, 2, 3, "split", split=True, ctl=dict(beta=0.3)),
    urow("beta_tensor_n330", 330, 1, 3, "split", split=True, ctl=dict(beta="tensor")),
    # ---------------- forced knobs: each against the truth, each with its own launch counts ----------------
    urow("split0_n449_m1", 449, 1, 3, "one", j=2, env={"LQP_UNROLL_SPLIT": "0"}),
    urow("scale_native0_n330", 330, 1, 3, "split", env={"LQP_UNROLL_SCALE_NATIVE": "0"}),
    urow("scale_native2_n330", 330, 2, 3, "split", env={"LQP_UNROLL_SCALE_NATIVE": "2"}),
    urow("native0_n200_m1", 200, 1, 2, "taped", env={"LQP_UNROLL_NATIVE": "0"}, lu=True,
         why="the taped loop of torch ops is its own forward (TorchLU per iteration): x is held to the bar, not to the bits of the "
             "functional solve"),
    # ---------------- the LU tape: k_unroll_sweep_lu (float64; m > 16, linsolve='lu', non-symmetric Q in float32) ----------------
    urow("lu64_n60_m1", 60, 1, 3, "lu64", dtype="f64"),
    urow("lu64_n256_m2", 256, 2, 2, "lu64", dtype="f64"),
    urow("lu64_n257_m2", 257, 2, 2, "lu64", dtype="f64"),
    urow("lu64_n450_m3", 450, 3, 2, "lu64", dtype="f64"),
    urow("lu32_m17_n200", 200, 17, 3, "lu32"),
    urow("lu32_linsolve_n300", 300, 1, 3, "lu32", ctl=LS_LU),
    urow("lu32_nonsym_n300", 300, 2, 3, "lu32", q="nonsym",
         why="the truth tapes the reference's own LU node (oracle RefLUSolve): its backward solves with the cached factor of M where the "
             "adjoint needs M^T -- 'only works for symmetric A' --, and the kernels return what the reference returns (against "
             "autograd through lu_solve dQ is off by 34 at scale 40)"),
    urow("lu32_N1024", 1008, 16, 2, "lu32", j=1, ctl=LS_LU),
    urow("lu32_N1025", 1008, 17, 2, "lu32", j=2),
    urow("lu64_N1024", 1022, 2, 2, "lu64", dtype="f64"),
    urow("lu64_N1025", 1024, 1, 2, "lu64", dtype="f64"),
    urow("lu32_n1025_m0", 1025, 0, 2, "lu32", why="above 1024 columns: the scaling kernels' slab loops take several passes"),
    urow("lu32_N2048", 2040, 8, 1, "lu32", j=14, K=3, why=K10),
    urow("lu32_N2049_m9", 2040, 9, 1, "lu32", j=1, K=3,
         why=K10 + "; n = 2049, m = 0 found no settled seed below 16 even at K = 3 (ratios up to 2.3): n = 2040, m = 9 instead"),
    # ---------------- tapes through rho events: lqp_boxqp_unroll_tape_segment / _finish ----------------
    urow("ev64_lo_n200_m1", 200, 1, 2, "ev64", dtype="f64", ctl=RHO_LO, K=K_EVENTS, n_factor=2),
    urow("ev64_hi_n200_m0", 200, 0, 2, "ev64", j=6, dtype="f64", ctl=RHO_HI, K=K_EVENTS, n_factor=3),
    urow("ev64_hi_noscale_n150_m2", 150, 2, 2, "ev64", j=2, dtype="f64", ctl=dict(RHO_HI, scale=False), K=K_EVENTS, n_factor=3),
    urow("ev64_lo_noscale_n150_m0", 150, 0, 2, "ev64", dtype="f64", ctl=dict(RHO_LO, scale=False), K=K_EVENTS, n_factor=2),
    urow("ev64_events0_n100_m1", 100, 1, 2, "taped", j=2, dtype="f64", ctl=RHO_HI, K=K_EVENTS, n_factor=3, lu=True,
         env={"LQP_UNROLL_EVENTS": "0"},
         why="the taped loop of torch ops is its own forward: x is held to the bar, not to the bits of the functional solve"),
    urow("ev32_grow_n330", 330, 1, 2, "ev32", ctl=dict(RHO_LO, **EV32), K=K_EV32, n_factor=2,
         why="K = 30 with check_solved = adaptive_rho_iter = 10: float32 and float64 tapes of K = 250 disagree on clamp decisions; "
             "rho = 0.01 grows at iteration 10 and is within the tolerance at 20"),
    urow("ev32_shrink_n330", 330, 1, 2, "ev32", j=3, ctl=dict(RHO_HI, **EV32), K=K_EV32, n_factor=2,
         why="K = 30 with check_solved = adaptive_rho_iter = 10; rho = 100 shrinks at iteration 10 and is within the tolerance at 20"),
]

ROW_BY_NAME = {r["name"]: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS), "duplicate row names"

KNOBS = ("LQP_UNROLL_SPLIT", "LQP_UNROLL_EVENTS", "LQP_UNROLL_NATIVE", "LQP_UNROLL_SCALE_NATIVE")
FORCED = {("LQP_UNROLL_SPLIT", "0"), ("LQP_UNROLL_EVENTS", "0"), ("LQP_UNROLL_NATIVE", "0"), ("LQP_UNROLL_SCALE_NATIVE", "0"),
          ("LQP_UNROLL_SCALE_NATIVE", "2")}

# boundaries of the unroll backward's selection code: (key, lower side, upper side[, row filter])
THRESHOLDS = {
    "n 128 | 129 (P.xchg: SPLIT_MINK)": ("n", 128, 129, "sym"),
    "Ks 4 | 5 (split sweep from Ks = 5)": ("Ks", 4, 5, "sym"),
    "Ks 5 | 6": ("Ks", 5, 6, "split"),
    "Ks 6 | 7": ("Ks", 6, 7, "split"),
    "Ks 7 | 8": ("Ks", 7, 8, "split"),
    "n 512 | 513 (SPD_MAXK: split sweep | streamed one-workgroup sweep)": ("n", 512, 513, "sym"),
    "n 1024 | 1025 (SPD_BIGK: symmetric sweep | LU tape)": ("n", 1024, 1025, "f32"),
    "N 1024 | 1025 float32 (EPT groups of k_unroll_sweep_lu)": ("N", 1024, 1025, "lu32"),
    "N 1024 | 1025 float64": ("N", 1024, 1025, "lu64"),
    "N 2048 | 2049": ("N", 2048, 2049, "lu32"),
    "m 1 | 2 one workgroup (k_unroll_sweep<1> | <SPD_MAXM>)": ("m", 1, 2, "one"),
    "m 1 | 2 at Ks = 8 (k_unroll_sweep_split<8, 1> | <8, SPD_MAXM>)": ("m", 1, 2, "split8"),
    "m 0 | 16 at Ks = 8": ("m", 0, 16, "split8"),
    "m 16 | 17 (SPD_MAXM: symmetric sweep | LU tape)": ("m", 16, 17, "f32"),
    "B cus/2 | cus/2 + 1 (shared_grid(B, 2) <= #CUs)": ("B", "cus//2", "cus//2 + 1", "n449"),
}
FILTERS = {
    "sym": lambda r: r["family"] in ("one", "split", "big"),
    "split": lambda r: r["family"] == "split",
    "split8": lambda r: r["family"] == "split" and ks(r["n"]) == 8,
    "one": lambda r: r["family"] == "one" and not r["env"],
    "f32": lambda r: r["dtype"] == "f32",
    "lu32": lambda r: r["family"] == "lu32",
    "lu64": lambda r: r["family"] == "lu64",
    "n449": lambda r: r["n"] == 449 and r["m"] == 1 and not r["env"],
}


def value(r, key):
    return ks(r["n"]) if key == "Ks" else r["n"] + r["m"] if key == "N" else r[key]


def dtype_of(r):
    return torch.float32 if r["dtype"] == "f32" else torch.float64


def beta_of(r, B, idx=None):
    """ctl["beta"] of the row: None, the float, or ("tensor") one value per problem, shape (B, 1) -- (len(idx), 1) for a sample."""
    beta = r["ctl"].get("beta")
    if beta != "tensor":
        return beta
    full = 0.15 + 0.5 * torch.arange(B, dtype=torch.float64).unsqueeze(1) / max(B, 1)
    return full if idx is None else full[torch.as_tensor(list(idx))]


def control(r, B, idx=None, dtype=None, K=None, **extra):
    """The pinned control of row r for the oracle (and, plus unroll / linsolve, for the HIP call)."""
    c = dict(eps_abs=1e-12, eps_rel=1e-12, max_iters=(r["K"] if K is None else K) + 1)
    for k in ("rho", "scale", "check_solved", "adaptive_rho_iter"):
        if k in r["ctl"]:
            c[k] = r["ctl"][k]
    beta = beta_of(r, B, idx)
    if beta is not None:
        c["beta"] = beta.to(dtype) if torch.is_tensor(beta) and dtype is not None else beta
    c.update(extra)
    return c


def make_control(r, B, idx=None, dtype=None, K=None, **extra):
    """`control` through the oracle's dict factory.  The factory writes its check_solved argument under the reference's misspelt
    key, which the solver does not read (control.py:8 against solve_box_qp_admm_torch.py:139): check_solved is set as a key."""
    from oracle import boxqp_oracle as O
    c = control(r, B, idx, dtype, K, **extra)
    check = c.pop("check_solved", None)
    d = O.make_control(**c)
    if check is not None:
        d["check_solved"] = check
    return d


def cotangent(r, B):
    g = torch.Generator().manual_seed(seed_of(r) + 1)
    return torch.randn(B, r["n"], 1, generator=g, dtype=torch.float64)


def tape(r, inp, dtype, cot, B, idx=None, K=None):
    """The oracle's unrolled tape of `inp` in `dtype`: -> ({x, dQ, ..., dub, n_factor}, trace with the clamp data)."""
    from oracle import boxqp_oracle as O
    d = [None if t is None else t.to(dtype) for t in inp]
    tr = {}
    x, g = O.unrolled_grad(cot.to(dtype), *d, make_control(r, B, idx, dtype, K), trace=tr,
                            lu_node="reference" if r["q"] == "nonsym" else None)
    return dict(g, x=x, n_factor=tr["n_factor"]), tr


def tie_mask(inp):
    """(B, n, 1) bool: lb == ub entries -- there the paths split the clamp gradient differently, dlb + dub is compared."""
    return inp[4] == inp[5]


def comparable(out, tie):
    """{x, dQ, dp, dA, db, dlb, dub off the ties, dlb + dub on them} of a tape / of the GPU run, float64 on the host."""
    c = lambda t: None if t is None else t.detach().cpu().double()
    res = {k: c(out.get(k)) for k in ("x", "dQ", "dp", "dA", "db")}
    dlb, dub = c(out["dlb"]), c(out["dub"])
    zero = torch.zeros_like(dlb)
    res["dlb"] = torch.where(tie, zero, dlb)
    res["dub"] = torch.where(tie, zero, dub)
    res["dlb+dub@tie"] = torch.where(tie, dlb + dub, zero)
    return res


def judge(r, hip, t32, t64, tie):
    """tier_table.compare, unchanged, on x and the six gradients."""
    return compare(r, comparable(hip, tie), None if t32 is None else comparable(t32, tie), comparable(t64, tie), keys=KEYS)


def settled(r, tr64, tr32=None):
    """Section 3 of the design: over every finite bound entry of every iteration of the float64 tape with x_k + u_k != bound,
    float32 rows: min |gap64| / |gap32 - gap64| (must reach R_MAX); float64 rows: min |gap64| / max(1, |x_k + u_k|_inf) (must reach
    F64_SETTLED).  gap = x_k + u_k - bound in the scaled space of the loop."""
    worst = math.inf
    for k, (w, lbs, ubs) in enumerate(tr64["clamps"]):
        for side, bnd in enumerate((lbs, ubs)):
            bnd = bnd.expand_as(w)
            use = torch.isfinite(bnd) & (w != bnd)
            if not bool(use.any()):
                continue
            gap = (w - bnd)[use].abs()
            if tr32 is not None:
                w32, l32, u32 = tr32["clamps"][k]
                g32 = (w32 - (l32, u32)[side].expand_as(w32)).double()
                dev = (g32[use] - (w - bnd)[use]).abs()
                worst = min(worst, float((gap / dev.clamp_min(1e-300)).min()))
            else:
                worst = min(worst, float(gap.min()) / max(1.0, float(w.abs().max())))
    return worst


def settled_ok(r, value):
    return value >= (R_MAX if r["dtype"] == "f32" else F64_SETTLED)


def row_tapes(r, cus=256, j=None):
    """(inputs of the sampled problems, cotangent, t64, t32 or None, trace64, trace32 or None) of row r at seed offset j."""
    rr = dict(r, j=r["j"] if j is None else j)
    B = batch(rr, cus)
    idx = sample(B)
    inp = inputs(rr, B, idx)
    cot = cotangent(rr, B)[torch.tensor(idx)]
    t64, tr64 = tape(rr, inp, torch.float64, cot, B, idx)
    t32 = tr32 = None
    if r["dtype"] == "f32":
        t32, tr32 = tape(rr, inp, torch.float32, cot, B, idx)
    return inp, cot, t64, t32, tr64, tr32
