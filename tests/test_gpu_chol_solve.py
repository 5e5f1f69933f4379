"""The block solves of the Cholesky backward (k_bwd_chol_solve): the register-resident solve against wg_chol_solve_n.  GPU only.

wg_chol_solve_reg (csrc/lqp_spd.hpp) keeps the factor of a free set of up to six 64-blocks in registers (two right-hand sides per
round; up to four blocks with four per round) and must give the bits of wg_chol_solve_n, which it replaces there: every value sees the
same operations in the same order.

1. lqp_debug_chol_solve runs either function on packed factors made here: a float64 Cholesky factor of a random SPD matrix (identity
   on the padding of the last block, as the backward pads), diagonal 64-blocks inverted, rounded once to float32.  Block counts
   Kb = 1, 2, 3, 5, 6 and 7, 8 (where both calls land in wg_chol_solve_n), free sets of 64 Kb - 63, 64 Kb - 12 and 64 Kb, all 21 in one
   launch; two right-hand sides per round with 1, 2, 3 of them, four with 1, 4, 5, 17.  The outputs are bit-equal, and the new one's
   error against the float64 solve of the same system is at most the old one's -- times 1.0: they are the same bits.
2. Through the layer, tests/fp_table.py's points with free sets on either side of 320 | 321 and 384 | 385 at n = 400, m = 1 and
   m = 16: the one-call and the prefactored backward give the same bits in all six gradients, and sit inside that table's comparator
   against its float64 oracle.
"""
import functools

import pytest
import torch

from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
import fp_table as FT
import tier_table as T

pytestmark = pytest.mark.gpu

KBS = (1, 2, 3, 5, 6, 7, 8)
NFS = [64 * k - d for k in KBS for d in (63, 12, 0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def sym_idx(i, j, K):
    return j * K - j * (j - 1) // 2 + (i - j)


@functools.lru_cache(maxsize=None)
def factor(nf, seed):
    """(A, packed): A the float64 SPD matrix padded with the identity to Kb blocks, packed its float32 factor as the backward's
    lower blocks (sym_blocks(Kb), 64, 64): L_ij below the diagonal, inv(L_jj) on it."""
    K = T.ks(nf)
    N = 64 * K
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(nf, nf, generator=g, dtype=torch.float64)
    A = torch.eye(N, dtype=torch.float64)
    A[:nf, :nf] = G @ G.T / nf + torch.eye(nf, dtype=torch.float64)
    Lb = torch.linalg.cholesky(A).view(K, 64, K, 64).permute(0, 2, 1, 3)
    packed = torch.zeros(K * (K + 1) // 2, 64, 64, dtype=torch.float64)
    for j in range(K):
        for i in range(j, K):
            packed[sym_idx(i, j, K)] = torch.linalg.inv(Lb[j, j]) if i == j else Lb[i, j]
    return A, packed.to(torch.float32)


@functools.lru_cache(maxsize=None)
def batch(nfs, Kmax, nrhs):
    """(packed (B, sym_blocks(Kmax), 64, 64), kb (B), V (B, nrhs, 64 Kmax), the float64 solutions) of the problems `nfs`"""
    B, N = len(nfs), 64 * Kmax
    packed = torch.zeros(B, Kmax * (Kmax + 1) // 2, 64, 64, dtype=torch.float32)
    g = torch.Generator().manual_seed(1000 + nrhs)
    V = torch.randn(B, nrhs, N, generator=g, dtype=torch.float32)
    X64 = torch.zeros(B, nrhs, N, dtype=torch.float64)
    for b, nf in enumerate(nfs):
        A, pk = factor(nf, 7 * nf + 1)
        packed[b, :pk.shape[0]] = pk
        Nb = A.shape[0]
        X64[b, :, :Nb] = torch.linalg.solve(A, V[b, :, :Nb].double().T).T
    return packed, torch.tensor([T.ks(nf) for nf in nfs], dtype=torch.int32), V, X64


def run(dev, packed, kb, V, Kmax, nr, which):
    lib = _lib.load()
    pk, kbd, Vd = packed.to(dev), kb.to(dev), V.to(dev)
    X = torch.full_like(Vd, float("nan"))
    _lib.check(lib.lqp_debug_chol_solve(_lib.stream_ptr(dev), V.shape[0], Kmax, _lib.ptr(pk), _lib.ptr(kbd), V.shape[1], nr, which,
                                        _lib.ptr(Vd), _lib.ptr(X)), "debug_chol_solve")
    torch.cuda.synchronize()
    return X.cpu()


def check(dev, nfs, Kmax, nr, nrhs):
    packed, kb, V, X64 = batch(tuple(nfs), Kmax, nrhs)
    old = run(dev, packed, kb, V, Kmax, nr, 0)
    new = run(dev, packed, kb, V, Kmax, nr, 1)
    bad = []
    for b, nf in enumerate(nfs):
        Nb = 64 * T.ks(nf)
        e_old = float((old[b].double() - X64[b]).abs().max())
        e_new = float((new[b].double() - X64[b]).abs().max())
        scale = float(X64[b].abs().max())
        print(f"chol_solve nr {nr} nrhs {nrhs} Kmax {Kmax} nf {nf}: err old {e_old:.3e} new {e_new:.3e} scale {scale:.3g} "
              f"equal {torch.equal(old[b], new[b])}")
        if not torch.equal(old[b], new[b]):
            bad.append(("bits", nf, float((old[b] - new[b]).abs().max())))
        if not e_new <= e_old * 1.0:                  # (the old function's own error on the same inputs: the same bits)
            bad.append(("error", nf, e_new, e_old))
        # the packing of this file, not the kernels: a float32 solve of a matrix with condition number below ~10 (G G^T / nf + I)
        # is far inside 1e-3 of the solution's size; a misplaced block is not
        if not e_old <= 1e-3 * scale:
            bad.append(("wg_chol_solve_n itself is off: the layout made here?", nf, e_old, scale))
        if bool(new[b, :, Nb:].any()) or not bool(torch.isfinite(new[b]).all()):
            bad.append(("past the last block", nf))
    assert not bad, bad


@pytest.mark.parametrize("nr,nrhs", [(2, 1), (2, 2), (2, 3), (4, 1), (4, 4), (4, 5), (4, 17)])
def test_register_solve_gives_the_bits_of_wg_chol_solve_n(dev, nr, nrhs):
    check(dev, NFS, 8, nr, nrhs)


@pytest.mark.parametrize("nr,nrhs", [(2, 2), (4, 5)])
@pytest.mark.parametrize("nfs,Kmax", [((372, 65, 448), 7), ((1, 384, 180), 6), ((256, 320, 129), 5)])
def test_three_block_counts_in_one_launch(dev, nfs, Kmax, nr, nrhs):
    check(dev, list(nfs), Kmax, nr, nrhs)


# ---- through the layer ----
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
@pytest.mark.parametrize("nfs", [(320, 321), (384, 385)])
def test_backward_on_either_side_of_the_block_limits(dev, nfs, m):
    """nf 320 | 321: five | six blocks (whole in registers | shared registers, two right-hand sides per round; wg_chol_solve_n with
    four); 384 | 385: six | seven blocks (the last resident count | wg_chol_solve_n)."""
    r = FT.row(f"chol_reg_nf{nfs[0]}_{nfs[1]}_m{m}_n400", 400, m, list(nfs))
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
