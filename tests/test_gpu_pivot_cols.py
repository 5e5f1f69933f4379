"""The pivot chain without its panels of padding (wg_pivot_block_mfma, COLS; csrc/lqp_spd.hpp).  GPU only.

A factorisation pads its last 64-block with the identity.  With LQP_PIV_COLS=1 (the default) the last pivot block of the backward's
look-ahead Cholesky stops behind the last real column; the panels of four columns that hold nothing but padding are run by no wave.
Eliminating a column of the identity changes no value (pivot 1, coefficients -0), so the factor must keep its bits.

1. lqp_debug_chol_factor runs the factorisation of k_bwd_chol_solve on matrices made here -- float64 G G^T / nf + I, padded with
   the identity, rounded once to float32 -- with 64 columns in every block (which = 0) and with the column count (which = 1), all
   free-set sizes in one launch of Kmax = 6, with float32 and with float16 tile products.  The blocks the problem does not use and the
   info words are NaN / -1 before the launch.  Every block of the factor and the info word are bit-equal, and the new factor's error
   against torch.linalg.cholesky in float64 is at most the old one's -- times 1.0.  With a real diagonal entry made negative both
   forms report that column, and never a column of the padding.
2. Through the layer, tests/fp_table.py's construction at n = 400, m = 1 and m = 16 with free sets 321, 324, 325, 352, 353: the one-call
   and the prefactored backward give the same bits in all six gradients and sit inside that table's comparator.
3. Forward and backward of the module at B = 8, m = 1, n = 129, 133, 161, 250, 500 (1, 5, 33, 58, 52 real columns in the last block) in two
   fresh processes, LQP_PIV_COLS=0 and =1: x, u, the iteration count and the gradients are bit-equal, and x sits inside
   tests/tier_table.py's comparator against its float64 solve.  (The resident sweep's last pivot step takes the column count too;
   the backward behind it is the Cholesky form.)
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
import fp_table as FT
import tier_table as T

pytestmark = pytest.mark.gpu

KMAX = 6
NFS = (1, 3, 4, 5, 31, 32, 33, 36, 60, 63, 64, 65, 68, 97, 128, 129, 321, 324, 325, 345, 352, 353, 384)
# (free-set size, column whose diagonal entry is made negative): in the last block's real columns, in an earlier block, right in
# front of the padding, the very first column
BAD = ((325, 322), (325, 100), (33, 32), (36, 31), (5, 0), (129, 128))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def sym_idx(i, j, K):
    return j * K - j * (j - 1) // 2 + (i - j)


@functools.lru_cache(maxsize=None)
def matrix(nf, bad_col=-1):
    """(A32 as float64, its lower blocks (sym_blocks(Kb), 64, 64) float32): G G^T / nf + I padded with the identity to Kb blocks"""
    K = T.ks(nf)
    N = 64 * K
    g = torch.Generator().manual_seed(11 * nf + 3)
    G = torch.randn(nf, nf, generator=g, dtype=torch.float64)
    A = torch.eye(N, dtype=torch.float64)
    A[:nf, :nf] = G @ G.T / nf + torch.eye(nf, dtype=torch.float64)
    if bad_col >= 0:
        A[bad_col, bad_col] = -1.0
    A32 = A.to(torch.float32)
    Ab = A32.view(K, 64, K, 64).permute(0, 2, 1, 3)
    blocks = torch.stack([Ab[i, j] for j in range(K) for i in range(j, K)])
    return A32.double(), blocks


@functools.lru_cache(maxsize=None)
def reference(nf):
    """the float64 factor of the float32 matrix in the layout of the kernel's output: L_ij below the diagonal, inv(L_jj) on it"""
    K = T.ks(nf)
    Lb = torch.linalg.cholesky(matrix(nf)[0]).view(K, 64, K, 64).permute(0, 2, 1, 3)
    return torch.stack([torch.linalg.inv(Lb[j, j]) if i == j else Lb[i, j] for j in range(K) for i in range(j, K)])


def run(dev, problems, f16, which):
    """problems: (nf, bad_col) each.  -> (packed (B, sym_blocks(KMAX), 64, 64), info (B)) after the launch"""
    B = len(problems)
    packed = torch.full((B, KMAX * (KMAX + 1) // 2, 64, 64), float("nan"), dtype=torch.float32)
    for b, (nf, bad_col) in enumerate(problems):
        blocks = matrix(nf, bad_col)[1]
        packed[b, :blocks.shape[0]] = blocks
    pk = packed.to(dev)
    nfd = torch.tensor([nf for nf, _ in problems], dtype=torch.int32, device=dev)
    info = torch.full((B,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().lqp_debug_chol_factor(_lib.stream_ptr(dev), B, KMAX, _lib.ptr(pk), _lib.ptr(nfd), f16, which, _lib.ptr(info)),
               "debug_chol_factor")
    torch.cuda.synchronize()
    return pk.cpu(), info.cpu()


@pytest.mark.parametrize("f16", [0, 1])
def test_column_count_keeps_the_bits_of_the_factor(dev, f16):
    problems = tuple((nf, -1) for nf in NFS)
    old, info_old = run(dev, problems, f16, 0)
    new, info_new = run(dev, problems, f16, 1)
    bad = []
    for b, nf in enumerate(NFS):
        nb = T.ks(nf) * (T.ks(nf) + 1) // 2
        ref = reference(nf)
        scale = float(ref.abs().max())
        e_old = float((old[b, :nb].double() - ref).abs().max())
        e_new = float((new[b, :nb].double() - ref).abs().max())
        same = torch.equal(old[b, :nb], new[b, :nb])
        print(f"chol_factor f16 {f16} nf {nf}: err old {e_old:.3e} new {e_new:.3e} scale {scale:.3g} info {int(info_old[b])} "
              f"{int(info_new[b])} equal {same}")
        if not same:
            bad.append(("bits", nf, float((old[b, :nb] - new[b, :nb]).abs().max())))
        if int(info_old[b]) != 0 or int(info_new[b]) != 0:
            bad.append(("info", nf, int(info_old[b]), int(info_new[b])))
        if not e_new <= e_old * 1.0:                  # (the 64-column run's own error on the same input: the same bits)
            bad.append(("error", nf, e_new, e_old))
        # the layout made in this file, not the kernels: the float32 factor of a matrix with condition number below ~10 (float16
        # tile products: two-half operands, ~2^-21) is far inside 1e-3 of the factor's size; a misplaced block is not
        if not e_old <= 1e-3 * scale:
            bad.append(("the 64-column factor itself is off: the layout made here?", nf, e_old, scale))
        for name, out in (("old", old), ("new", new)):
            if not bool(torch.isnan(out[b, nb:]).all()):
                bad.append(("a block the problem does not own was written", name, nf))
    assert not bad, bad


@pytest.mark.parametrize("f16", [0, 1])
def test_a_pivot_that_is_not_positive_is_reported_at_its_column(dev, f16):
    _, info_old = run(dev, BAD, f16, 0)
    _, info_new = run(dev, BAD, f16, 1)
    bad = []
    for b, (nf, col) in enumerate(BAD):
        print(f"chol_factor f16 {f16} nf {nf} negative diagonal at {col}: info old {int(info_old[b])} new {int(info_new[b])}")
        if int(info_old[b]) != col + 1 or int(info_new[b]) != col + 1:
            bad.append((nf, col, int(info_old[b]), int(info_new[b])))
        if int(info_old[b]) > nf or int(info_new[b]) > nf:
            bad.append(("a column of the padding was reported", nf, int(info_old[b]), int(info_new[b])))
    assert not bad, bad


# ---- through the layer: backward ----
def _call(entry, r, gpu_pt):
    cot, rest = gpu_pt[0], gpu_pt[1:]
    want = dict(dQ=True, dp=True, dA=r["m"] > 0, db=r["m"] > 0, dlb=True, dub=True)
    _lib.profile(enable=True, reset=True)
    try:
        if entry == "chol":
            out = SB._fp_backward(cot, *rest, want, linsolve=2)
        else:
            out = SB._fp_backward_run(SB._fp_backward_prepare(*rest, want, linsolve=2, prefactor=True), cot)
        torch.cuda.synchronize()
        used = _lib.profile()
    finally:
        _lib.profile(enable=False)
    return dict(zip(FT.GRADS, out[:6])), tuple(used[c][1] for c in FT.PROF_CLASSES)


@pytest.mark.parametrize("m", [1, 16])
def test_backward_with_few_real_columns_in_the_last_block(dev, m):
    """Six blocks with 1, 4, 5, 32, 33 real columns in the last one: a single panel, a full panel, one column of the second panel,
    wave 0's last panel, wave 3's first."""
    r = FT.row(f"chol_pivcols_m{m}_n400", 400, m, [321, 324, 325, 352, 353])
    pt = FT.point(r, r["B"])
    gpu_pt = tuple(t.to(dev) if torch.is_tensor(t) else t for t in pt)
    one, form1 = _call("chol", r, gpu_pt)
    two, form2 = _call("chol_pre", r, gpu_pt)
    bad = []
    if form1 != FT.FORMS["chol"] or form2 != FT.FORMS["chol_pre"]:
        bad.append(("form", form1, form2))
    for k in FT.GRADS:
        if (one[k] is None) != (two[k] is None) or (one[k] is not None and not torch.equal(one[k], two[k])):
            bad.append(("two phases changed bits", k))
    t64 = FT.oracle(pt, torch.float64)
    t32 = FT.oracle(pt, torch.float32)
    for entry, grads in (("chol", one), ("chol_pre", two)):
        res = FT.compare(r, {k: (None if v is None else v.cpu()) for k, v in grads.items()}, t32, t64)
        if set(res) != {k for k in FT.GRADS if t64[k] is not None}:
            bad.append(("compared", entry, sorted(res)))
        for k, rec in res.items():
            print(f"{r['name']} {entry} {k}: err {rec['err']:.3e} budget {rec.get('budget', float('nan')):.3e} "
                  f"ratio {rec.get('ratio', float('nan')):.3g} bar {rec['bar']:.3e} ok {rec['ok']}")
            if not rec["ok"]:
                bad.append(("value", entry, k, rec))
    assert not bad, (r["name"], bad)


# ---- through the layer: forward (and the backward behind it) in fresh processes ----
SWEEP_NS = (129, 133, 161, 250, 500)


def _sweep_row(n):
    return T.row(f"pivcols_sweep_n{n}", n, 1, 8, ctl=dict(linsolve=2), sig=T.SPD)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import torch
import lqp_py_amd as L
from oracle import boxqp_oracle as O
import tier_table as T
import test_gpu_pivot_cols as me
dev = torch.device("cuda:0")
out = {}
for n in me.SWEEP_NS:
    r = me._sweep_row(n)
    inp = T.inputs(r, r["B"])
    args = [None if t is None else t.to(dev) for t in inp]
    ctl = O.make_control(**T.control(r), linsolve=r["ctl"]["linsolve"])
    sol = L.torch_solve_box_qp(*args, dict(ctl))
    Qg, pg = args[0].clone().requires_grad_(True), args[1].clone().requires_grad_(True)
    x = L.SolveBoxQP(control=dict(ctl, sync=True))(Qg, pg, args[2], args[3], args[4], args[5])
    g = torch.Generator().manual_seed(n)
    x.backward(torch.randn(r["B"], n, 1, generator=g).to(dev))
    torch.cuda.synchronize()
    out[n] = dict(x=sol["x"].cpu(), u=sol["u"].cpu(), iter=int(sol["iter"]), linsolve_used=int(sol["_stats"]["linsolve_used"]),
                  xm=x.detach().cpu(), dQ=Qg.grad.cpu(), dp=pg.grad.cpu())
torch.save(out, sys.argv[3])
"""


def _child(tmp_path, value):
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / f"piv_cols_{value}.pt")
    env = dict(os.environ, LQP_PIV_COLS=value)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _CHILD, os.path.dirname(here), here, path]
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, (value, done.stdout[-2000:], done.stderr[-2000:])
    return torch.load(path)


def test_knob_changes_no_bit_of_forward_and_backward(dev, tmp_path):
    off = _child(tmp_path, "0")
    on = _child(tmp_path, "1")
    bad = []
    for n in SWEEP_NS:
        r = _sweep_row(n)
        a, b = off[n], on[n]
        for k in ("x", "u", "xm", "dQ", "dp"):
            if not torch.equal(a[k], b[k]):
                bad.append(("bits", n, k, float((a[k] - b[k]).abs().max())))
        if a["iter"] != b["iter"] or a["iter"] != r["K"]:
            bad.append(("iter", n, a["iter"], b["iter"], r["K"]))
        if a["linsolve_used"] != 2 or b["linsolve_used"] != 2:
            bad.append(("not the symmetric x-update", n, a["linsolve_used"], b["linsolve_used"]))
        inp = T.inputs(r, r["B"])
        t64 = T.oracle(r, inp, torch.float64)
        t32 = T.oracle(r, inp, torch.float32)
        rec = T.compare(r, dict(x=b["x"]), t32, t64, keys=("x",))["x"]
        print(f"piv_cols sweep n {n}: iter {b['iter']} x err {rec['err']:.3e} budget {rec['budget']:.3e} bar {rec['bar']:.3e} ok {rec['ok']}")
        if not rec["ok"]:
            bad.append(("value", n, rec))
    assert not bad, bad
