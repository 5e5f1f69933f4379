"""tests/lu_table.py proved on the CPU, before any GPU sees it: LAPACK returns every row's planted factor and pivots bit for bit in
float64 AND in float32, the plain getf2 with the kernels' holder maps agrees, P A' = L U holds in integers, the rows cover every
panel kind and every tie class of every kernel instantiation (with a winner that is not the lowest holder), a wrong tie rule
changes the pivots of every row that claims a tie, and expect_kernel is what the restated selection gives on 256 and 304 CUs."""
import functools

import numpy as np
import pytest
import torch

import lu_table as T


def _exact_product(A, LU, ipiv):
    """P A == L U in integers (everything scaled by 2): row interchanges as LAPACK applies them, the product column by column of L
    over its non-zeros only."""
    N = A.shape[0]
    A2 = 2.0 * A
    L2 = 2.0 * np.tril(LU, -1) + 2.0 * np.eye(N)
    U = np.triu(LU)
    for M in (A2, L2, U):
        if not np.array_equal(M, np.rint(M)):
            return False
    A2, L2, U = A2.astype(np.int64), L2.astype(np.int64), U.astype(np.int64)
    for j in range(N):
        p = int(ipiv[j]) - 1
        if p != j:
            A2[[j, p]] = A2[[p, j]]
    acc = np.zeros((N, N), dtype=np.int64)
    for k in range(N):
        rows = np.nonzero(L2[:, k])[0]
        cols = np.nonzero(U[k])[0]
        acc[np.ix_(rows, cols)] += np.outer(L2[rows, k], U[k, cols])
    return bool(np.array_equal(acc, A2))


@functools.lru_cache(maxsize=None)
def summary(name):
    """Everything this module asserts about one row, computed once (the matrices are dropped again: 4096^2 doubles each)."""
    r = T.ROW_BY_NAME[name]
    A, LU, ipiv = T.planted(r)
    pb, ntp, _ = T.geometry(r)
    out = dict(amax=float(A.abs().max()), lapack={}, pb=pb)
    for b in range(r["B"]):
        for dt in (torch.float64, torch.float32):
            lu, piv, info = torch.linalg.lu_factor_ex(A[b].to(dt))
            out["lapack"][(b, dt)] = (bool(torch.equal(lu, LU[b].to(dt))), bool(torch.equal(piv, ipiv[b])), int(info))
            # the casts lose nothing
            assert torch.equal(A[b].to(dt).double(), A[b]) and torch.equal(LU[b].to(dt).double(), LU[b])
    h = T.holders(r)
    out["getf2"] = bool(np.array_equal(h["LU"], LU[0].numpy())) and bool(np.array_equal(h["ipiv"], ipiv[0].numpy()))
    out["info"] = h["info"]
    out["product"] = all(_exact_product(A[b].numpy(), LU[b].numpy(), ipiv[b].numpy()) for b in range(r["B"]))
    out["kinds"] = T.panel_kinds(h, pb)
    out["classes"] = T.tie_classes(h)
    out["nonlowest"] = T.tie_classes(h, nonlowest=True)
    out["zero_ties"] = [t for t in h["ties"] if t["zero"]]
    out["wrong"] = {rule: T.getf2(A[0].numpy(), pb, ntp, rule=rule, stop_at=ipiv[0].numpy())["diff"] for rule in ("lowthread", "highpos")}
    return out


@pytest.mark.parametrize("name", [r["name"] for r in T.ROWS])
def test_row_is_exact(name):
    r = T.ROW_BY_NAME[name]
    s = summary(name)
    want_info = 0 if r["zero"] is None else min(r["zero"]) + 1
    for key, (lu_ok, piv_ok, info) in s["lapack"].items():
        assert lu_ok and piv_ok, f"LAPACK does not return the planted factor / pivots of {name} {key}: factor {lu_ok}, pivots {piv_ok}"
        assert info == want_info, (name, key, info)
    assert s["getf2"], "the plain getf2 disagrees with the plant"
    assert s["info"] == want_info
    assert s["product"], "P A' != L U in integers"
    assert s["amax"] < 2 ** 10
    if r["zero"] is not None:
        # the zero pivot is the product of cancellation, not a zero input column; the whole live column ties at zero there
        A = T.planted(r)[0][0]
        for j in r["zero"]:
            assert j == 0 or float(A[:, j].abs().max()) > 0, (name, j)
        if min(r["zero"]) < r["N"] - 1:
            assert any(t["step"] == min(r["zero"]) for t in s["zero_ties"])


@pytest.mark.parametrize("name", [r["name"] for r in T.REGULAR if r["N"] > 32])
def test_wrong_tie_rule_changes_the_pivots(name):
    """A table that cannot see the bug fails: "the lowest thread wins" and "the largest position wins" must both give other
    pivots on every row that claims a tie with a winner that is not the lowest holder."""
    s = summary(name)
    assert s["nonlowest"], f"{name} plants no tie whose winner is not the lowest holder"
    assert s["wrong"]["lowthread"] is not None and s["wrong"]["highpos"] is not None, s["wrong"]


def _groups():
    g = {}
    for r in T.REGULAR:
        g.setdefault((r["expect_kernel"], r["dtype"]), []).append(r)
    return g


@pytest.mark.parametrize("key", sorted(_groups()))
def test_every_instantiation_meets_every_kind_and_class(key):
    rows = _groups()[key]
    pb = summary(rows[0]["name"])["pb"]
    kernel = rows[0]["kernel"]
    kinds, classes, nonlowest = set(), set(), set()
    for r in rows:
        s = summary(r["name"])
        kinds |= s["kinds"]
        classes |= s["classes"]
        nonlowest |= s["nonlowest"]
    assert kinds >= T.kinds_possible(pb), (key, sorted(T.kinds_possible(pb) - kinds))
    assert classes >= T.classes_possible(kernel), (key, sorted(T.classes_possible(kernel) - classes))
    assert nonlowest >= T.classes_possible(kernel), (key, sorted(T.classes_possible(kernel) - nonlowest))


def test_families_and_dtypes():
    seen = {(r["kernel"], r["dtype"]) for r in T.REGULAR}
    want = {(k, d) for k in T.FAMILIES for d in ("f32", "f64")} - {("tall", "f64")}
    assert seen >= want, sorted(want - seen)
    assert any(r["expect_kernel"] == "big/pb4/r4" for r in T.REGULAR) and any(r["expect_kernel"].endswith("r2") for r in T.REGULAR)
    inst = {r["expect_kernel"] for r in T.REGULAR if r["dtype"] == "f32"}
    assert inst >= {f"one/pb{pb}/{u}/512" for pb in (16, 32) for u in ("mfma", "valu")} | {"one/pb8/valu/512", "one/pb8/valu/1024",
                                                                                             "one/pb16/mfma/1024"}, sorted(inst)
    assert {r["expect_kernel"] for r in T.REGULAR if r["dtype"] == "f64" and r["kernel"] == "one"} >= {"one/pb16/mfma/512", "one/pb8/mfma/1024"}
    # every family that can take a singular row takes one, first / last column and a double zero among them
    sing = {(r["kernel"], r["dtype"]) for r in T.SINGULAR}
    assert sing >= want - {("tall", "f64")}, sorted(want - sing)
    assert any(len(r["zero"]) == 2 for r in T.SINGULAR) and any(r["zero"] == (0,) for r in T.SINGULAR)
    assert any(r["zero"] == (r["N"] - 1,) for r in T.SINGULAR)


def test_both_sides_of_every_threshold():
    def k(N, dt, B=1):
        rows = [r for r in T.REGULAR if r["N"] == N and r["dtype"] == dt and r["B"] == B]
        assert rows, (N, dt, B)
        return rows[0]["expect_kernel"]
    assert any(r["N"] <= 64 for r in T.REGULAR) and any(64 < r["N"] <= 128 for r in T.REGULAR)          # one wave | more
    assert k(95, "f32", 2).startswith("one/") and k(96, "f32", 2) == "two/pb32"
    assert k(47, "f64", 2).startswith("one/") and k(48, "f64", 2) == "two/pb16"
    for dt in ("f32", "f64"):
        assert any(r["N"] == 512 and r["dtype"] == dt and r["expect_kernel"].endswith("/512") for r in T.REGULAR)
        assert k(513, dt).endswith("/1024") and k(1024, dt).endswith("/1024")
        assert k(1025, dt, 1).startswith("big/") and k(1025, dt, 2).startswith("wide/")
        assert k(2048, dt, 1).endswith("/r2") and k(2048, dt, 2).startswith("wide/")
    assert k(2049, "f32").endswith("/r4") or k(2049, "f32") == "tall/pb4"
    assert {r["expect_kernel"] for r in T.REGULAR if r["N"] in (2049, 4096)} == {"big/pb4/r4", "tall/pb4"}
    assert any(r["N"] == 1 for r in T.REGULAR) and any(r["N"] == 32 and r["dtype"] == "f32" for r in T.REGULAR)
    assert any(r["N"] == 16 and r["dtype"] == "f64" for r in T.REGULAR)


@pytest.mark.parametrize("cus", T.CUS)
def test_expect_kernel_is_the_restated_selection(cus):
    for r in T.ROWS:
        s = T.select(r["N"], r["B"], r["dtype"], r["env"], cus=cus)
        assert s["name"] == r["expect_kernel"] and s["kernel"] == r["kernel"], (r["name"], s)
    # the knobs of the rows mean what the rows take them to mean
    assert T.select(300, 1, "f32")["kernel"] == "two" and T.select(300, 1, "f32", {"LQP_LU2": "0"})["name"] == "one/pb32/mfma/512"
    assert T.select(300, 1, "f32", {"LQP_LU2": "0", "LQP_LU_PB": "8", "LQP_LU_MFMA": "1"})["name"] == "one/pb8/valu/512"
    assert T.select(300, 1, "f32", {"LQP_LU2": "0", "LQP_LU_NT": "1024"})["name"] == "one/pb16/mfma/1024"
    assert T.select(300, 1, "f32", {"LQP_LU2": "0", "LQP_LU_NT": "1024", "LQP_LU_PB": "32"})["name"] == "one/pb16/mfma/1024"
    assert T.select(1500, 1, "f32")["kernel"] == "wide" and T.select(1500, cus, "f32")["kernel"] == "big"
    assert T.select(3000, 1, "f32", {"LQP_LU_WIDE": "0"})["name"] == "big/pb4/r4"
    with pytest.raises(ValueError):
        T.select(2049, 1, "f64")
