"""control['alpha'] without a GPU: the truth of tests/relax_table.py, what its rows can see, and the rules of the new key -- the
ValueErrors of the Python layer, the struct field, the argument checks of lqp_boxqp_forward."""
import ctypes
import math
import os
import re

import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import each_table as E
import relax_table as RT
import tier_table as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256                      # (only the batch size of the rows that are an expression of the CU count depends on it)
KEYS = ("x", "z", "u", "lams", "nus", "rho")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", list(RT.STOPS))
def test_the_restatement_at_alpha_one_is_the_oracle(case, dtype):
    """alpha = 1.0 passed to the oracle (solve_relaxed) against the argument absent, bit for bit"""
    n, B, seed = case
    qp = O.create_qp_data(n, B, seed=seed, dtype=dtype)
    want = O.solve_box_qp(*qp, O.make_control(**RT.STOP_CONTROL))
    got = RT.stop_truth(n, B, seed, 1.0, dtype)
    assert got["iter"] == want["iter"]
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("key", list(RT.ROWS))
def test_every_row_sees_the_plain_step(key):
    """The oracle's plain step (alpha = 1) FAILS the row's bar against the relaxed truth by at least 100 x on x: a kernel that
    ignored the factor, or one of its three sites that did, cannot pass."""
    r = RT.ROWS[key]
    idx, t32, t64 = RT.row_truth(key, CUS)
    assert t64["iter"] == r["K"] and (t32 is None or t32["n_factor"] == t64["n_factor"])
    sub = T.inputs(r, T.batch(r, CUS), idx)
    plain = RT.truth(r, sub, torch.float32 if r["dtype"] == "f32" else torch.float64, alpha=1.0)
    rec = T.compare(r, plain, t32, t64)["x"]
    print(key, "plain step: |x - t64| =", rec["err"], "bar", rec["bar"], "bars", rec["err"] / rec["bar"])
    assert rec["err"] >= 100 * rec["bar"], rec


def test_rows_keep_the_tier_rows_they_are_named_after():
    assert {r["alpha"] for r in RT.ROWS.values()} == {RT.ALPHA, RT.ALPHA_UNDER}
    assert len(RT.ROWS) == len(RT.TIERS) + len(RT.UNDER)
    for key, r in RT.ROWS.items():
        base = T.ROW_BY_NAME[r["name"]]
        assert all(r[k] == base[k] for k in base if k not in ("K", "flip", "why")), key
        assert r["K"] == (RT.K_EVENT if r["name"] == "events_lo_n330" else RT.K_PINNED)
        assert (r["R"], r["F"]) == (T.R_DEFAULT, T.F_DEFAULT)
    # the event row: past the event, and the event refactorises in every truth (its signature says n_factor = 2)
    ev = RT.ROWS[f"events_lo_n330-a{RT.ALPHA}"]
    _, t32, t64 = RT.row_truth(f"events_lo_n330-a{RT.ALPHA}", CUS)
    assert ev["K"] > 100 and t32["n_factor"] == t64["n_factor"] == ev["sig"]["n_factor"] == 2


@pytest.mark.parametrize("case", list(RT.STOPS))
def test_iteration_counts_of_the_stopped_solves(case):
    plain, relaxed = RT.STOPS[case]
    for dtype in (torch.float32, torch.float64):
        assert RT.stop_truth(*case, 1.0, dtype)["iter"] == plain
        assert RT.stop_truth(*case, RT.ALPHA, dtype)["iter"] == relaxed
    assert relaxed < plain


def test_each_row_counts_agree_in_both_dtypes_and_differ_from_the_plain_ones():
    i32 = [s["iter"] for s in RT.each_truth(torch.float32)]
    i64 = [s["iter"] for s in RT.each_truth(torch.float64)]
    assert i32 == i64 and i32 != E.ROWS[RT.EACH_ROW]["iters"], (i32, i64)


@pytest.mark.parametrize("name", list(RT.GRAD_ROWS))
@pytest.mark.parametrize("backward", ["fixed_point", "kkt"])
def test_gradient_rows_have_no_active_set_flip_between_the_dtypes(name, backward):
    r = RT.GRAD_ROWS[name]
    idx, t32, t64 = RT.row_truth(name, CUS, "GRAD_ROWS")
    B = T.batch(r, CUS)
    sub = T.inputs(r, B, idx)
    cot = RT.cot_of(r, B, torch.float64)[idx]
    g32 = RT.truth_grads(r, sub, t32, cot, torch.float32, backward)
    g64 = RT.truth_grads(r, sub, t64, cot, torch.float64, backward)
    for k in T.GRADS:
        scale = max(1.0, float(g64[k].abs().max()))
        assert float((g32[k].double() - g64[k]).abs().max()) <= 1e-3 * scale, (k, backward)


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python layer
def test_resolve_control_takes_numbers_and_one_element_tensors():
    assert SB.resolve_control({}, 10)["alpha"] == 1.0
    assert SB.resolve_control(dict(alpha=1.6), 10)["alpha"] == 1.6
    assert SB.resolve_control(dict(alpha=1), 10)["alpha"] == 1.0
    assert SB.resolve_control(dict(alpha=torch.tensor([0.5])), 10)["alpha"] == 0.5
    assert L.box_qp_control(alpha=1.6)["alpha"] == 1.6 and "alpha" not in L.box_qp_control()


@pytest.mark.parametrize("bad", [0.0, 2.0, -0.5, 2.5, math.nan, math.inf, "1.6", None, True, [1.6], torch.tensor([1.0, 1.6])])
def test_a_bad_alpha_is_a_value_error_at_the_call(bad):
    """... before anything looks at the tensors: none is given"""
    ctl = L.box_qp_control(alpha=bad)
    with pytest.raises(ValueError, match="alpha"):
        L.torch_solve_box_qp(None, None, None, None, None, None, ctl)
    with pytest.raises(ValueError, match="alpha"):
        SB.SolveBoxQPLayer.apply(None, None, None, None, None, None, ctl)
    with pytest.raises(ValueError, match="alpha"):
        SB.check_stop(dict(ctl, stop='each'))
    with pytest.raises(ValueError, match="alpha"):
        SB.resolve_control(ctl, 10)


def test_unroll_refuses_a_relaxed_step():
    for ctl in (L.box_qp_control(alpha=1.6, unroll=True), L.box_qp_control(alpha=torch.tensor(0.5), unroll=True)):
        with pytest.raises(ValueError, match="unroll"):
            L.torch_solve_box_qp(None, None, None, None, None, None, ctl)
        with pytest.raises(ValueError, match="unroll"):
            L.SolveBoxQP(control=ctl)(None, None, None, None, None, None)
    SB.check_stop(L.box_qp_control(alpha=1.0, unroll=True))         # (the plain step is what the tape replays)
    SB.check_stop(L.box_qp_control(alpha=1.6))


def _struct(control):
    like = torch.zeros(1)
    return SB._control_struct(control, 4, 100, like, True, True, False)[2]


def test_struct_field_and_the_bytes_of_an_absent_key():
    absent, one, relaxed = _struct(L.box_qp_control()), _struct(L.box_qp_control(alpha=1.0)), _struct(L.box_qp_control(alpha=1.6))
    assert bytes(absent) == bytes(one)
    assert absent.alpha == 0.0 and relaxed.alpha == 1.6
    assert bytes(relaxed)[:_lib.BoxQPCtrl.alpha.offset] == bytes(absent)[:_lib.BoxQPCtrl.alpha.offset]
    # the field is the struct's last: every earlier offset is what it was
    assert _lib.BoxQPCtrl.alpha.offset + 8 == ctypes.sizeof(_lib.BoxQPCtrl) and _lib.BoxQPCtrl._fields_[-1][0] == "alpha"
    assert _lib.BoxQPCtrl.host_report.offset + 8 == _lib.BoxQPCtrl.alpha.offset


def _header_struct_bytes(text):
    """sizeof(lqp_boxqp_ctrl) from the header's own declarations (int32_t: 4; double, pointers: 8, each on its own alignment)"""
    body = re.search(r"typedef struct lqp_boxqp_ctrl \{(.*?)\} lqp_boxqp_ctrl;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, last = 0, None
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        size = 4 if decl.startswith("int32_t") else 8
        assert size == 4 or decl.startswith("double") or "*" in decl, decl
        off = (off + size - 1) // size * size + size
        last = decl
    return (off + 7) // 8 * 8, last


def test_header_binding_and_library_agree_on_abi_17():
    text = open(os.path.join(REPO, "include", "lqp_amd.h")).read()
    lib = _lib.load()
    assert lib.lqp_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define LQP_ABI_VERSION (\d+)", text).group(1)) == 17
    size, last = _header_struct_bytes(text)
    assert last == "double alpha"
    assert size == ctypes.sizeof(_lib.BoxQPCtrl) == lib.lqp_boxqp_ctrl_bytes()


def test_forward_refuses_a_bad_alpha_before_it_touches_anything():
    """Dummy pointers that are never dereferenced and a workspace of 0 bytes: a call whose arguments pass ends at the workspace
    check (2), in front of the first use of a device; a bad alpha ends before that (1)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)

    def call(**fields):
        ctl = _lib.BoxQPCtrl(max_iters=10, check_solved=1, **fields)
        return lib.lqp_boxqp_forward(None, 0, 1, 4, 0, fake, fake, None, None, fake, fake, ctypes.byref(ctl), None,
                                     fake, fake, fake, fake, None, fake, None, fake, 0)
    assert call() == 2 and call(alpha=1.0) == 2 and call(alpha=1.6) == 2 and call(alpha=0.5, reserved2=2 | 4 | 8) == 2
    assert call(alpha=1.0, reserved2=1) == 2 and call(reserved2=1) == 2
    for bad in (2.5, 2.0, -0.5, math.nan, math.inf, -math.inf):
        assert call(alpha=bad) == 1, bad
    assert call(alpha=1.6, reserved2=1) == 1 and call(alpha=0.5, reserved2=1 | 4) == 1
