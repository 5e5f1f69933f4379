"""control['stop'] = 'each' without a GPU: the table of tests/each_table.py is a fair test (heterogeneous, and decided by the
problems, not by rounding), the combinations that cannot mean anything are refused at the call, the default is untouched in the
control struct, and the C ABI carries the new entry."""
import ctypes
import os
import re

import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from lqp_py_amd.unrolled import unrolled_solve_box_qp
from oracle import boxqp_oracle as O
import each_table as ET

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(ET.ROWS))
def test_rows_are_heterogeneous_and_not_decided_by_rounding(name):
    row = ET.ROWS[name]
    i32, i64 = ET.solo_iters(name, torch.float32), ET.solo_iters(name, torch.float64)
    check = O.default_check_interval(row["n"])
    print(name, "iterations per problem: float32", i32, "float64", i64)
    # the float32 and the float64 oracle agree on EVERY problem's count (no exclusions), and the table holds it
    assert i32 == i64 == row["iters"]
    # at least three distinct counts (a batch of two: two), one problem optimal at its first or second check
    assert len(set(i64)) >= min(3, row["B"])
    assert min(i64) <= check
    cap = row["control"]["max_iters"] - 1
    assert row["control"]["max_iters"] <= 1500 and [i for i, c in enumerate(i64) if c == cap] == row["never"]
    # every problem keeps finite bounds on both sides
    qp = ET.inputs(row)
    assert bool(torch.isfinite(qp[4]).all()) and bool(torch.isfinite(qp[5]).all()) and bool((qp[4] < qp[5]).all())
    if name == "chunk_n20":      # (what the row is for: a check at every iteration, and a problem that stops behind the first 512)
        assert check == 1 and any(512 < c < cap for c in i64)
        # ... whose verdict has room against float32 rounding: the same counts with the tolerance 0.2 % tighter and looser
        for f in (0.998, 1.002):
            for dt in (torch.float32, torch.float64):
                ctl = ET.control(row, eps_abs=row["control"]["eps_abs"] * f, eps_rel=row["control"]["eps_rel"] * f)
                moved = [int(O.solve_box_qp(*(t[i:i + 1] for t in ET.inputs(row, dt)), ctl, bounds=(True, True))["iter"]) for i in range(row["B"])]
                assert moved == row["iters"], (f, dt, moved)
    if row["adapts"] is not None:
        a32, a64 = ET.solo_adapts(name, torch.float32), ET.solo_adapts(name, torch.float64)
        print(name, "adapts rho: float32", a32, "float64", a64)
        assert a32 == a64 == row["adapts"]
        assert any(a64) and not all(a64)
        # the event the adapting problems went through is the first possible one, and they were still running at it
        ar_iter = O.resolve_control(ET.control(row), row["n"]).adaptive_rho_iter
        assert all(i >= ar_iter for i, a in zip(i64, a64) if a)
    else:
        assert not any(ET.solo_adapts(name, torch.float64))


def test_the_truth_differs_from_the_batch_rule():
    """What the rows are for: under the reference's rule (torch.all) the early problems iterate on, so their batch results are not
    their solo results -- a solver that ignored control['stop'] could not pass the GPU comparison."""
    row = ET.ROWS["small_n100"]
    whole = O.solve_box_qp(*ET.inputs(row, torch.float64), ET.control(row))
    assert whole["iter"] == max(row["iters"])
    solo = ET.solo("small_n100", torch.float64)
    moved = [float((whole["x"][i] - solo[i]["x"][0]).abs().max()) for i in range(row["B"])]
    print("|x of the batch - x of the problem alone|", moved)
    # the problems that stop early iterate on in the batch: their batch iterate is not the one they stopped with
    assert sum(m > 1e-9 for i, m in enumerate(moved) if row["iters"][i] < max(row["iters"])) >= 3
    assert all(m == 0.0 for i, m in enumerate(moved) if row["iters"][i] == max(row["iters"]))


def _cpu_qp():
    return O.create_qp_data(8, 2, seed=0)


@pytest.mark.parametrize("extra,where", [
    (dict(stop='each', unroll=True), "functional"),
    (dict(stop='each', unroll=True), "module"),
    (dict(stop='each', dist_strict_stop=True), "functional"),
    (dict(stop='each', dist_strict_stop=True), "sharded"),
    (dict(stop='each', _check_hook=lambda c, i: None), "layer"),
    (dict(stop='every'), "functional"),
    (dict(stop=1), "module"),
])
def test_combinations_that_cannot_mean_anything_raise_at_the_call(extra, where):
    """ValueError before anything touches a device: the inputs are CPU tensors, which the solve itself would refuse with a
    RuntimeError (no CPU path) -- the ValueError comes first."""
    control = L.box_qp_control(**extra)
    qp = _cpu_qp()
    with pytest.raises(ValueError, match="stop"):
        if where == "functional":
            L.torch_solve_box_qp(*qp, control)
        elif where == "module":
            L.SolveBoxQP(control=control)(*qp)
        elif where == "sharded":
            from lqp_py_amd.dist import ShardedBoxQP
            ShardedBoxQP(control)(*qp)
        else:
            SB.SolveBoxQPLayer.apply(*qp, control)


def test_unrolled_entry_refuses_each():
    qp = _cpu_qp()
    with pytest.raises(ValueError, match="stop"):
        unrolled_solve_box_qp(*qp, SB.resolve_control(dict(stop='each'), 8), True, True)


def test_a_check_hook_passed_beside_the_dict_is_refused_too():
    with pytest.raises(ValueError, match="stop"):
        SB._forward_solve(*_cpu_qp(), dict(stop='each'), check_hook=lambda c, i: None)


def _struct_bytes(control):
    like = torch.zeros(1, dtype=torch.float32)
    _r, _rho, ctl, _rt, _bt = SB._control_struct(control, 4, 16, like, True, True, False)
    return ctypes.string_at(ctypes.addressof(ctl), ctypes.sizeof(ctl))


def test_default_and_absent_key_resolve_to_the_same_control_struct():
    base = dict(eps_abs=1e-5, eps_rel=1e-5, rho=0.5)
    assert _struct_bytes(dict(base)) == _struct_bytes(dict(base, stop='all'))
    # ... and 'each' differs from them in nothing the struct caches: the bit is a field of the call (reserved2 bit 3)
    assert _struct_bytes(dict(base, stop='each')) == _struct_bytes(dict(base))
    assert SB.resolve_control(dict(base), 16)['stop'] == 'all' and SB.resolve_control(dict(base, stop='each'), 16)['stop'] == 'each'


def test_abi_carries_the_new_entry():
    header = open(os.path.join(REPO, "include", "lqp_amd.h")).read()
    assert re.search(r"int lqp_boxqp_problem_iters\(void\* stream, int dtype, int B, int n, int m,\s*const void\* workspace, "
                     r"size_t workspace_bytes, int32_t\* iters_out\);", header)
    assert "bit 3 (ABI 14)" in header and int(re.search(r"#define LQP_ABI_VERSION (\d+)", header).group(1)) >= 14
    assert "lqp_boxqp_problem_iters" in _lib.SYMBOLS and _lib.ABI_VERSION >= 14
    lib = _lib.load()
    assert hasattr(lib, "lqp_boxqp_problem_iters")
    # refused before anything touches a device: bad arguments, and a workspace no 'each' forward has used
    buf = (ctypes.c_char * 64)()
    out = (ctypes.c_int32 * 4)()
    assert lib.lqp_boxqp_problem_iters(None, 0, 4, 16, 0, None, 0, out) == 1
    assert lib.lqp_boxqp_problem_iters(None, 0, 4, 16, 0, buf, 64, None) == 1
    assert lib.lqp_boxqp_problem_iters(None, 0, 4, 16, 0, buf, 64, out) == 1
    # the per-problem words sit behind everything else: every offset of the layout is what it was
    so, sb, io, ib = (ctypes.c_size_t() for _ in range(4))
    assert lib.lqp_boxqp_forward_layout(0, 4, 16, 0, ctypes.byref(so), ctypes.byref(sb), ctypes.byref(io), ctypes.byref(ib)) == 0
    assert (so.value, sb.value) == (0, 64)
    # ... and the workspace grew by exactly the per-problem block behind what was there (4 int32 per problem at the next multiple of the
    # carve's 256 bytes; `before` = the size every build before ABI 14 gave, which ends in 256 spare bytes)
    for (dt, B, n, m), before in {(0, 4, 16, 0): 288000, (0, 128, 500, 1): 420562432, (1, 8, 70, 3): 3131904, (0, 2, 1030, 1): 28185856}.items():
        assert lib.lqp_boxqp_forward_layout(dt, B, n, m, ctypes.byref(so), ctypes.byref(sb), ctypes.byref(io), ctypes.byref(ib)) == 0
        assert (so.value, sb.value, io.value, ib.value) == (0, 64, 33024, 4 * B)
        assert lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m) == (before - 256 + 255) // 256 * 256 + 16 * B + 256, (dt, B, n, m)
