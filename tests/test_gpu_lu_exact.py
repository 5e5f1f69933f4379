"""Every row of tests/lu_table.py on the GPU: lu_layer.lu_factor must return the planted factor and pivots EXACTLY (torch.equal, no
tolerance).  This is not a measurement: every intermediate of these factorisations is exactly representable in float32, so any
correct partial-pivoting LU with the first-index tie rule returns these bits whatever the order of its sums, on the matrix cores
or not (tests/test_lu_table.py shows LAPACK doing so on the CPU in both precisions).  The rows plant swaps, ties and zero pivots
where the kernels' interchange bookkeeping is at work: see tests/lu_table.py.  GPU only.

Singular rows: the factorisation goes on past the zero pivot as getf2 does (the planted factor again, bit for bit), and lu_factor
raises with the planted FIRST zero column, the same message from every kernel family.

That the kernel a row names ran: the cycle counters of lqp_debug_set_lu_counters tell the launch shapes apart -- four words per
matrix from k_lu_factor (lqp_lu.hpp), sixteen from lqp_lu2.hpp and lqp_lu_wide.hpp (eight used by the latter), none from
k_lu_factor_big (the same body with several panel rows per thread, given no counter block); which
instantiation of the one-workgroup kernel ran rests on expect_kernel (tests/test_lu_table.py checks it against the restated
selection), see each row's `why`.

The solves: rhs = A' X with integer |X| <= 4, three columns, through lu_solve and TorchLU, with the planted factor and with the
GPU's own, against X under the comparator and the default R, F of the `solve` family of tests/direct_table.py (t64 = X, t32 =
float32 LAPACK's solve on the CPU).
"""
import pytest
import torch

from lqp_py_amd import _lib, lu_layer
import lu_table as T
import tier_table as TT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _raw_factor(A):
    """lqp_lu_factor_batched without lu_factor's raise: (LU, pivots, info) and what the counters say ran."""
    lib = _lib.load()
    dev = A.device
    B, N = A.shape[0], A.shape[1]
    dt = _lib.dtype_code(A)
    LU = A.clone().contiguous()
    piv = torch.zeros((B, N), dtype=torch.int32, device=dev)
    info = torch.full((B,), -99, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.lqp_lu_factor_workspace_bytes(dt, B, N)), dtype=torch.uint8, device=dev)
    dbg = torch.zeros(16 * B + 16, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib.lqp_debug_set_lu_counters(_lib.ptr(dbg))
    try:
        with torch.cuda.device(dev):
            st = lib.lqp_lu_factor_batched(_lib.stream_ptr(dev), dt, B, N, _lib.ptr(LU), _lib.ptr(piv), _lib.ptr(info), _lib.ptr(ws),
                                           ws.numel())
        torch.cuda.synchronize()
    finally:
        lib.lqp_debug_set_lu_counters(None)
    _lib.check(st, "lu_factor")
    c = dbg.cpu()
    if not bool(c.any()):
        shape = "none"                                   # k_lu_factor_big
    elif bool(c[4 * B:].any()):
        shape = "sixteen" if all(int(c[16 * b + 7]) > 0 for b in range(B)) else "?"       # lqp_lu2.hpp | lqp_lu_wide.hpp: [7] total
    else:
        shape = "four" if all(int(c[4 * b + 3]) > 0 for b in range(B)) else "?"           # lqp_lu.hpp: [3] total
    return LU, piv, info, shape


SHAPE = {"one": "four", "two": "sixteen", "wide": "sixteen", "tall": "sixteen", "big": "none"}


def _setenv(monkeypatch, r):
    for k in ("LQP_LU2", "LQP_LU_WIDE", "LQP_LU_WIDE_MIN", "LQP_LU_PB", "LQP_LU_MFMA", "LQP_LU_NT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)


def _inputs(r, dev):
    A, LU_want, ipiv_want = T.planted(r)
    dt = T.DTYPES[r["dtype"]]
    return A.to(dt).to(dev), LU_want.to(dt), ipiv_want


def _check_factor(r, LU, piv, LU_want, ipiv_want):
    ok = torch.equal(piv.cpu(), ipiv_want) and torch.equal(LU.cpu(), LU_want)
    assert ok, f"{r['name']} ({r['expect_kernel']}): not the planted factorisation\n" + T.explain(r, LU, piv)


@pytest.mark.parametrize("name", [r["name"] for r in T.REGULAR])
def test_factor_is_the_planted_one(name, dev, monkeypatch):
    r = T.ROW_BY_NAME[name]
    _setenv(monkeypatch, r)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert T.select(r["N"], r["B"], r["dtype"], r["env"], cus=cus)["name"] == r["expect_kernel"]
    A, LU_want, ipiv_want = _inputs(r, dev)
    LU, piv, info, shape = _raw_factor(A)
    assert shape == SHAPE[r["kernel"]], f"{name}: counters of shape {shape!r}, the row names {r['expect_kernel']}"
    assert info.cpu().tolist() == [0] * r["B"]
    _check_factor(r, LU, piv, LU_want, ipiv_want)
    # the public entry point: the same bits, LAPACK's conventions (int32, 1-based)
    LU2, piv2 = lu_layer.lu_factor(A)
    assert piv2.dtype == torch.int32 and LU2.dtype == A.dtype
    _check_factor(r, LU2, piv2, LU_want, ipiv_want)


@pytest.mark.parametrize("name", [r["name"] for r in T.SINGULAR])
def test_zero_pivot_is_reported_and_factoring_goes_on(name, dev, monkeypatch):
    r = T.ROW_BY_NAME[name]
    _setenv(monkeypatch, r)
    A, LU_want, ipiv_want = _inputs(r, dev)
    j = min(r["zero"])
    LU, piv, info, shape = _raw_factor(A)
    assert shape == SHAPE[r["kernel"]], f"{name}: counters of shape {shape!r}, the row names {r['expect_kernel']}"
    assert info.cpu().tolist() == [j + 1] * r["B"], f"{name}: info {info.cpu().tolist()}, the first zero pivot is column {j} (0-based)"
    _check_factor(r, LU, piv, LU_want, ipiv_want)
    with pytest.raises(RuntimeError) as e:
        lu_layer.lu_factor(A)
    assert str(e.value) == (f"lqp_py_amd.lu_factor: (Batch element 0): U[{j + 1},{j + 1}] is zero and using it on lu_solve would result "
                            "in a division by zero.")


SOLVE_ROWS = [r["name"] for r in T.REGULAR if r["N"] > 1]


@pytest.mark.parametrize("name", SOLVE_ROWS)
def test_solves_with_the_planted_and_the_gpu_factor(name, dev, monkeypatch):
    r = T.ROW_BY_NAME[name]
    _setenv(monkeypatch, r)
    A, LU_want, ipiv_want = _inputs(r, dev)
    B, N = r["B"], r["N"]
    g = torch.Generator().manual_seed(N)
    X = torch.randint(-4, 5, (B, N, 3), generator=g).double()
    rhs64 = T.planted(r)[0] @ X                                  # small integers and halves: exact, and exact in float32
    rhs = rhs64.to(A.dtype).to(dev)
    assert torch.equal(rhs.cpu().double(), rhs64)
    t32 = {"x": torch.linalg.solve(A.cpu().float(), rhs.cpu().float()).double()} if r["dtype"] == "f32" else None
    LUg, pivg = lu_layer.lu_factor(A)
    bar = dict(dtype=r["dtype"], R=TT.R_DEFAULT, F=TT.F_DEFAULT)
    bad = []
    for tag, (LU, piv) in (("planted", (LU_want.to(dev), ipiv_want.to(dev))), ("gpu", (LUg, pivg))):
        outs = {"lu_solve": lu_layer.lu_solve(LU, piv, rhs), "TorchLU": lu_layer.TorchLU(LU=LU, P=piv)(A, rhs)}
        for how, x in outs.items():
            assert x.shape == rhs.shape and x.dtype == rhs.dtype
            rec = TT.compare(bar, {"x": x.cpu().double()}, t32, {"x": X}, keys=("x",))["x"]
            print(f"lu_exact:{name} {tag} {how}: err {rec['err']:.3e} budget {rec.get('budget', float('nan')):.3e} bar {rec['bar']:.3e} ok {rec['ok']}")
            if not rec["ok"]:
                bad.append((tag, how, rec))
    assert not bad, bad
