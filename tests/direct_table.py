"""The entry points that do not run the ADMM loop, as data (no GPU needed to import this module): the cached LU solve
(lu_layer.lu_factor / lu_solve / _PackedFactor: k_pack and k_packed_solve), TorchLU / TorchLULayer, the equality-constrained and
the unconstrained QP with their gradients (k_kkt_build, the LU chain, k_kkt_unpack, k_outer_grads), OptNet's equality-only branch
and the box-QP layer on a batch without any finite bound (rho = 0, one solve, iter == 0, the backward with rho = 0).
tests/test_gpu_direct.py runs every row on the GPU; tests/test_direct_table.py checks, without a GPU, that the rows sit on both
sides of every edge of that code, that the oracle is the dense algebra written out, that the budgets are usable and that the
comparator sees errors.

Inputs: one well-conditioned KKT-like family for every row, built in float64 and rounded ONCE to the row's dtype:
G ~ randn(n + 8, n), Q = G'G / (n + 8) + 0.05 I, A ~ randn(m, n), M = [[Q, A'], [A, 0]]; right-hand sides and cotangents randn.
cond(M) is 1e2 .. 3e3 over the rows (tests/test_direct_table.py bounds it by 1e4), the zero block makes the pivoting real.

The truth is always the CPU oracle (oracle.boxqp_oracle) in float64 on the rounded values, the budget the same function in float32:
float32 rows |hip - t64| <= R |t32 - t64| + F scale, float64 rows |hip - t64| <= 1e-9 scale (tier_table.compare).

Row fields:
  name, family ("solve" | "lulayer" | "eqcon" | "uncon" | "optnet" | "layer0"), n, m, N = n + m, B, dtype ("f32" | "f64")
  rhs      solve / lulayer: the form of the right-hand side, see RHS_FORMS ("k3t": (B,N,3) as the transposed view of a (B,3,N) tensor)
  factor   solve: "hip" (lu_layer.lu_factor) | "torch" (torch.linalg.lu_factor on the CPU, packed by k_pack)
  q        "sym" | "nonsym" (Q with a small antisymmetric part: the LU layer's same-factor backward is then not the adjoint)
  singular eqcon: (problem, row of A) set to zero -- an exactly zero pivot whatever the rounding; the call must raise
  j        offset of the row's seed (tier_table.seed_of), found by a search: the m = n rows, where an unlucky square A leaves cond(M) > 1e4
  env      LQP_* overrides; same=True: the run under `env` must give the bits of the run without it
  ctl      layer0: scale, launch_mode, sync
  tier     layer0: the LU tier the forward must report having run, see TIERS (sol["_stats"])
  R, F, why as in tests/tier_table.py
"""
import math

import torch

import tier_table as T

FAMILIES = ("solve", "lulayer", "eqcon", "uncon", "optnet", "layer0")
RHS_FORMS = {"2d": 1, "k1": 1, "k2": 2, "k3": 3, "k17": 17, "k3t": 3}      # form -> number of right-hand sides
RING = {"f32": 8, "f64": 6}          # csrc/lqp_trsv.hpp: LQP_PF, LQP_PF64 -- blocks in flight of k_packed_solve
GROUP = {"f32": 8, "f64": 4}         # csrc/lqp_trsv.hpp: pack_group -- diagonal blocks k_pack stages at a time
# what sol["_stats"] of a no-bound forward must say per tier: (mode_used, loop_workgroups) -- None: as many as the chip gives (> 2)
TIERS = {"dense2": (2, 2), "densew": (2, None), "loop1": (1, 1), "wide": (2, None)}
SPLIT_MAXB = 128                     # csrc/lqp_amd.hip: small_batch_split -- two workgroups per factor up to this batch size


def m_of(N):
    """Equality rows of a `solve` / `lulayer` row's matrix, by its size: (63, 3) ... (1025, 25)."""
    return 0 if N < 8 else max(3, N // 41)


def row(name, family, size, B=3, dtype="f32", rhs="k3", factor="hip", env=None, ctl=None, R=T.R_DEFAULT, F=T.F_DEFAULT,
        same=False, why=None, q="sym", singular=None, j=0, tier=None):
    if isinstance(size, tuple):
        n, m = size
    elif family == "uncon":
        n, m = size, 0
    else:
        m = m_of(size)
        n = size - m
    return dict(name=f"{name}_{dtype}", family=family, n=n, m=m, N=n + m, B=B, dtype=dtype, rhs=rhs, factor=factor, env=dict(env or {}),
                ctl=dict(ctl or {}), R=R, F=F, same=same, why=why, q=q, singular=singular, j=j, tier=tier)


def both(*a, **k):
    return [row(*a, dtype="f32", **k), row(*a, dtype="f64", **k)]


SPLIT2_OFF = dict(env={"LQP_SPLIT2": "0"}, same=True,
                  why="the second workgroup per factor takes the U half of the pack: the same bits (measured for the pack by the "
                      "bwd_split2off row of tests/tier_table.py)")
SCALED = dict(scale=True)

ROWS = [
    # ---------------- solve: block and alignment edges (K = ceil(N / 64); vector loads need N % 4 == 0) ----------------
    *both("solve_n1", "solve", 1, rhs="k1"),
    *both("solve_n63", "solve", 63),
    *both("solve_n64", "solve", 64),
    *both("solve_n128", "solve", 128),
    *both("solve_n129", "solve", 129),
    # ---------------- solve: every form of the right-hand side at N = 65 (two blocks, scalar loads) and N = 200 ----------------
    *[r for N in (65, 200) for form in ("2d", "k1", "k3", "k17", "k3t") for r in both(f"solve_n{N}_{form}", "solve", N, rhs=form)],
    # ---------------- solve: the prefetch ring (8 blocks float32, 6 float64) against the K (K + 1) blocks, nrhs = 3 ----------------
    row("solve_ring_n448", "solve", 448, why="K = 7: 56 = 7 x 8 blocks, no padding step; the ring wraps into the next right-hand side"),
    row("solve_ring_n192", "solve", 192, why="K = 3: 12 blocks padded to 16"),
    row("solve_ring_n192", "solve", 192, dtype="f64", why="K = 3: 12 = 2 x 6 blocks, no padding step"),
    row("solve_ring_n256", "solve", 256, dtype="f64", why="K = 4: 20 blocks padded to 24"),
    # ---------------- solve: the second staging group of k_pack (K > 8 float32, K > 4 float64) ----------------
    row("solve_n257", "solve", 257, dtype="f64", why="K = 5 > 4"),
    # ---------------- solve: k_pack on one workgroup per factor (B > 128, or LQP_SPLIT2=0) ----------------
    *both("solve_n65_b129", "solve", 65, B=129),
    *both("solve_n130_b129", "solve", 130, B=129),
    *both("solve_n65_split2off", "solve", 65, **SPLIT2_OFF),
    *both("solve_n130_split2off", "solve", 130, **SPLIT2_OFF),
    # ---------------- solve: the LU tiers' size edges ----------------
    *both("solve_n512", "solve", 512),
    *both("solve_n513", "solve", 513, why="float32: K = 9 > 8, the second staging group"),
    *both("solve_n1024", "solve", 1024, B=2, rhs="k2"),
    *both("solve_n1025", "solve", 1025, B=2, rhs="k2"),
    row("solve_n2048", "solve", 2048, B=1, rhs="k2", dtype="f64"),
    row("solve_n2049", "solve", 2049, B=1, rhs="k1"),
    row("solve_n4096", "solve", 4096, B=1, rhs="k1"),
    # ---------------- solve: a LAPACK factor packed by k_pack ----------------
    *both("solve_n65_torch", "solve", 65, factor="torch"),
    *both("solve_n130_torch", "solve", 130, factor="torch"),
    *both("solve_n513_torch", "solve", 513, factor="torch"),
    # ---------------- the LU layer: cached (TorchLU) and un-cached (TorchLULayer.apply), forward and backward ----------------
    *both("lulayer_n65_2d", "lulayer", 65, rhs="2d"),
    *both("lulayer_n65_k3", "lulayer", 65, rhs="k3"),
    *both("lulayer_n200_2d", "lulayer", 200, rhs="2d"),
    *both("lulayer_n200_k3", "lulayer", 200, rhs="k3"),
    *both("lulayer_nonsym_n130", "lulayer", 130, q="nonsym"),
    # ---------------- the equality-constrained QP: x, nus, dQ, dp, dA, db ----------------
    *both("eqcon_n1_m1", "eqcon", (1, 1)),
    *both("eqcon_n60_m4", "eqcon", (60, 4)),
    *both("eqcon_n60_m5", "eqcon", (60, 5)),
    row("eqcon_n64_m64", "eqcon", (64, 64), j=5, why="m = n: A is square, cond(M) ~ cond(A)^2; j: the first draws with cond(M) < 2e3"),
    row("eqcon_n64_m64", "eqcon", (64, 64), dtype="f64", j=3, why="m = n: A is square, cond(M) ~ cond(A)^2; j: the first draws with cond(M) < 2e3"),
    *both("eqcon_n100_m17", "eqcon", (100, 17)),
    row("eqcon_n130_m65", "eqcon", (130, 65), R=5.0,
        why="measured: dQ 4.03, dp 3.72, x 3.50 times the float32 budget (k_packed_solve multiplies by explicit inverses of the "
            "diagonal blocks where LAPACK substitutes)"),
    row("eqcon_n130_m65", "eqcon", (130, 65), dtype="f64"),
    *both("eqcon_n500_m12", "eqcon", (500, 12)),
    *both("eqcon_n500_m13", "eqcon", (500, 13)),
    row("eqcon_n1020_m5", "eqcon", (1020, 5), B=2),
    *both("eqcon_singular_n130_m3", "eqcon", (130, 3), B=4, singular=(2, 1)),
    # ---------------- the unconstrained QP: x, dQ, dp ----------------
    *[r for n in (1, 64, 65, 130, 513) for r in both(f"uncon_n{n}", "uncon", n)],
    # ---------------- OptNet, equality-only branch, autograd on Q, p, A, b ----------------
    row("optnet_n130_m3", "optnet", (130, 3)),
    row("optnet_n70_m2", "optnet", (70, 2), dtype="f64"),
    # ---------------- the box-QP layer without any finite bound: one row per LU tier such a batch can reach ----------------
    row("layer0_dense2_n128_m1", "layer0", (128, 1), ctl=SCALED, tier="dense2"),
    row("layer0_densew_n257_m2", "layer0", (257, 2), ctl=SCALED, tier="densew"),
    row("layer0_loop1_n600_m2", "layer0", (600, 2), ctl=dict(SCALED, launch_mode=1), tier="loop1", R=5.0,
        why="measured: dp of backward='kkt' 4.38 times the float32 budget, every other output below 2.1 (the KKT backward is one "
            "packed solve without a refinement step: explicit inverses of the diagonal blocks where LAPACK substitutes)"),
    row("layer0_wide_n1025_m0", "layer0", (1025, 0), B=2, ctl=SCALED, tier="wide"),
    row("layer0_noscale_n257_m2", "layer0", (257, 2), ctl=dict(scale=False), tier="densew"),
    row("layer0_dense2_n128_m0", "layer0", (128, 0), ctl=SCALED, tier="dense2"),
    row("layer0_nosync_n257_m2", "layer0", (257, 2), ctl=dict(SCALED, sync=False), tier="densew"),
    row("layer0_dense2_n128_m1", "layer0", (128, 1), dtype="f64", ctl=SCALED, tier="dense2"),
    row("layer0_densew_n257_m2", "layer0", (257, 2), dtype="f64", ctl=SCALED, tier="densew"),
]

ROW_BY_NAME = {r["name"]: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS), "duplicate row names"


def rows_of(family, singular=False):
    return [r for r in ROWS if r["family"] == family and (r["singular"] is not None) == singular]


def dtype_of(r):
    return torch.float32 if r["dtype"] == "f32" else torch.float64


def nrhs(r):
    return RHS_FORMS[r["rhs"]]


def ring_exact(r):
    """Do the K (K + 1) blocks of the packed factor fill the prefetch ring without a padding step?"""
    K = T.ks(r["N"])
    return K * (K + 1) % RING[r["dtype"]] == 0


def pack_groups(r):
    """Trips of k_pack's loop over the staged diagonal blocks."""
    return -(-T.ks(r["N"]) // GROUP[r["dtype"]])


def pack_split(r):
    """Does k_pack run on two workgroups per factor (L half, U half)?"""
    return r["B"] <= SPLIT_MAXB and r["env"].get("LQP_SPLIT2", "1") != "0"


def shape_rhs(r, base):
    """The row's form of a contiguous (B, N, nrhs) tensor (on any device): the same values."""
    form = r["rhs"]
    if form == "2d":
        return base.reshape(base.shape[0], base.shape[1])
    if form == "k3t":
        return base.transpose(1, 2).contiguous().transpose(1, 2)
    return base


def as3(t):
    return t.unsqueeze(2) if t is not None and t.dim() == 2 else t


def _problem(r, i):
    """(Q, A) of problem i in float64."""
    n, m = r["n"], r["m"]
    g = torch.Generator().manual_seed(T.seed_of(r) * 7919 + i)
    G = torch.randn(n + 8, n, generator=g, dtype=torch.float64)
    Q = G.T @ G / (n + 8) + 0.05 * torch.eye(n, dtype=torch.float64)
    Q = 0.5 * (Q + Q.T)
    if r["q"] == "nonsym":
        S = torch.randn(n, n, generator=g, dtype=torch.float64)
        Q = Q + 0.02 * (S - S.T)
    A = torch.randn(m, n, generator=g, dtype=torch.float64) if m else None
    if r["singular"] is not None and r["singular"][0] == i:
        A[r["singular"][1]] = 0.0
    return Q, A


def kkt(Q, A):
    """[[Q, A'], [A, 0]] (Q alone without equality rows)."""
    from oracle import boxqp_oracle as O
    return Q if A is None else O.kkt_matrix(Q, A)


def inputs(r):
    """The row's inputs in the row's dtype: Q, A (None when m = 0), M, p (B,n,1), b (B,m,1), cot (B,n,1), and for solve / lulayer
    `base` (B,N,nrhs): the right-hand side -- shape_rhs gives its form -- and `gbase`, the cotangent of the solve, shaped alike."""
    dt = dtype_of(r)
    B, n, m, N = r["B"], r["n"], r["m"], r["N"]
    parts = [_problem(r, i) for i in range(B)]
    Q = torch.stack([pt[0] for pt in parts]).to(dt)
    A = torch.stack([pt[1] for pt in parts]).to(dt) if m else None
    g = torch.Generator().manual_seed(T.seed_of(r) + 1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dt)
    inp = dict(Q=Q, A=A, M=kkt(Q, A), p=rnd(B, n, 1), b=rnd(B, m, 1) if m else None, cot=rnd(B, n, 1))
    if r["family"] in ("solve", "lulayer"):
        inp.update(base=rnd(B, N, nrhs(r)), gbase=rnd(B, N, nrhs(r)))
    return inp


def _cast(inp, dtype, *keys):
    return [None if inp[k] is None else inp[k].to(dtype) for k in keys]


def _unbounded(p):
    return torch.full_like(p, -math.inf), torch.full_like(p, math.inf)


def layer0_control(r, **extra):
    """The oracle's control of a layer0 row (the HIP call adds launch_mode / sync / backward)."""
    from oracle import boxqp_oracle as O
    return O.make_control(scale=r["ctl"].get("scale", True), **extra)


def point(r, inp):
    """What the gradient FUNCTIONS (torch_solve_qp_eqcon_grad, torch_solve_qp_uncon_grad, torch_solve_box_qp_grad) are evaluated at:
    the oracle's forward solution in the ROW's dtype -- x, nus (and for layer0 u = 0, lams = 0).  The GPU call, the budget and the
    truth receive the same numbers.  Computed once per `inp`."""
    from oracle import boxqp_oracle as O
    if "point" not in inp:
        Q, p, A, b = _cast(inp, dtype_of(r), "Q", "p", "A", "b")
        if r["family"] == "layer0":
            sol = O.solve_box_qp(Q, p, A, b, *_unbounded(p), layer0_control(r))
            inp["point"] = dict(x=sol["x"], nus=sol["nus"], u=torch.zeros_like(p), lams=torch.zeros_like(torch.cat((p, p), 1)))
        else:
            sol = O.solve_qp_eqcon(Q, p, A, b) if r["m"] else O.solve_qp_uncon(Q, p)
            inp["point"] = dict(x=sol["x"], nus=sol.get("nus"))
    return inp["point"]


def truth(r, inp, dtype, hook=None):
    """{output: tensor} of the row's family from the CPU oracle in `dtype`.  `hook` (tests of the comparator) maps the converted
    input dict to a wrong one.
      solve     x = linalg.solve(M, rhs)
      lulayer   x = lu_solve(lu_factor(M), rhs), (dA, db) = lu_layer_backward of the cotangent gbase
      eqcon     x, nus = solve_qp_eqcon; dQ, dp, dA, db = solve_qp_eqcon_grad(cot, point)
      uncon     x = solve_qp_uncon; dQ, dp = solve_qp_uncon_grad(cot, point)
      optnet    x = solve_qp_eqcon and the gradients at that x, nus (what autograd through the layer gives)
      layer0    x, z, u, lams, nus = solve_box_qp without bounds; fp.*: solve_box_qp_grad at that solution with its rho = 0;
                kkt.*: solve_box_qp_grad_kkt at that solution; direct.*: solve_box_qp_grad(cot, point, rho = 0), all six"""
    from oracle import boxqp_oracle as O
    d = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in inp.items() if k != "point"}
    pt = {k: (None if v is None else v.to(dtype)) for k, v in point(r, inp).items()} if r["family"] in ("eqcon", "uncon", "layer0") else None
    if hook is not None:
        d = hook(d)
    Q, p, A, b, M, cot = (d[k] for k in ("Q", "p", "A", "b", "M", "cot"))
    fam = r["family"]
    if fam == "solve":
        return dict(x=torch.linalg.solve(M, d["base"]))
    if fam == "lulayer":
        LU, piv = O.lu_factor(M)
        x = O.lu_solve(LU, piv, d["base"])
        dA, db = O.lu_layer_backward(LU, piv, x, d["gbase"])
        return dict(x=x, dA=dA, db=db)
    if fam == "uncon":
        dQ, dp = O.solve_qp_uncon_grad(cot, pt["x"], Q)
        return dict(x=O.solve_qp_uncon(Q, p)["x"], dQ=dQ, dp=dp)
    if fam in ("eqcon", "optnet"):
        sol = O.solve_qp_eqcon(Q, p, A, b)
        at = sol if fam == "optnet" else pt
        dQ, dp, dA, db = O.solve_qp_eqcon_grad(cot, at["x"], at["nus"], Q, A)
        return dict(x=sol["x"], nus=sol["nus"], dQ=dQ, dp=dp, dA=dA, db=db)
    assert fam == "layer0"
    lb, ub = _unbounded(p)
    sol = O.solve_box_qp(Q, p, A, b, lb, ub, layer0_control(r))
    assert sol["iter"] == 0 and sol["rho"] == 0
    out = {k: sol[k] for k in ("x", "z", "u", "lams", "nus") if sol[k] is not None}
    names = ("dQ", "dp", "dA", "db", "dlb", "dub")
    fp = O.solve_box_qp_grad(cot, sol["x"], sol["u"], sol["lams"], sol["nus"], Q, A, lb, ub, sol["rho"])
    kk = O.solve_box_qp_grad_kkt(cot, sol["x"], sol["lams"], sol["nus"], Q, A, lb, ub)
    di = O.solve_box_qp_grad(cot, pt["x"], pt["u"], pt["lams"], pt["nus"], Q, A, lb, ub, 0)
    for tag, g, keep in (("fp", fp, 4), ("kkt", kk, 4), ("direct", di, 6)):      # (the module hands out dQ, dp, dA, db)
        out.update({f"{tag}.{k}": v for k, v in zip(names[:keep], g) if v is not None})
    return out


def compare(r, hip, t32, t64, keys=None):
    """tier_table.compare over the outputs the truth holds (2-D solutions as (B,N,1)); an output the truth holds and `hip` lacks is
    an error of its own (the callers check the set of compared keys)."""
    keys = tuple(t64) if keys is None else keys
    f = lambda d: None if d is None else {k: as3(v) for k, v in d.items()}
    return T.compare(r, f(hip), f(t32), f(t64), keys=keys)
