"""control['infeasible'] on the GPU: every row of tests/infeas_table.py against its truth (solve_detect of each problem on its own).

For every row, with the key set: `status` and `iters` are the table's lists exactly (the float32 and the float64 truth agree on them
and every verdict stands clear of the threshold: tests/test_infeas_table.py), the row runs on the kernel family it is named for,
the feasible problems are bit-identical to the same call without the key, and a flagged problem's x is the truth's iterate of the
detecting check at the bar of tests/test_gpu_each.py.  Then the layer: 'raise' (at the call, and late through synchronize() when
the call did not wait), 'flag' (gradient rows of flagged problems exactly zero, the others bit-identical to the call without the
key), batches in which nothing is infeasible, and that nothing depends on what the enlarged workspace held.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
import each_table as ET
import infeas_table as IT
import memharness as H

pytestmark = pytest.mark.gpu

ROWS = list(IT.ROWS)
GRADS = ("dQ", "dp", "dA", "db", "dlb", "dub")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def gpu_control(row, dev, **extra):
    ctl = dict(row["control"], stop='each', **extra)
    if row.get("rho_b") is not None:
        ctl["rho"] = torch.tensor(row["rho_b"], dtype=row["dtype"], device=dev).view(-1, 1, 1)
    return L.box_qp_control(**ctl)


def gpu_inputs(row, dev):
    return tuple(None if t is None else t.to(dev) for t in IT.inputs(row, row["dtype"]))


def schedule(monkeypatch, name):
    """the chunk row runs the host-driven persistent schedule, as tests/test_gpu_each.py reaches it"""
    if name == "chunk_n20":
        monkeypatch.setenv("LQP_SYNC_PLAN", "0")
        monkeypatch.setattr(SB, "_SYNC_SPLIT", False)


_SOLVED = {}


def solved(name, dev, monkeypatch, key):
    """-> (solution on the host, last_forward_status) of the row with control['infeasible'] = key (None: absent), computed once"""
    if (name, key) not in _SOLVED:
        row = IT.ROWS[name]
        schedule(monkeypatch, name)
        sol = L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row, dev, **({} if key is None else dict(infeasible=key))))
        st = SB.last_forward_status(dev)
        last = L.last_problem_status(dev)
        assert last is sol["status"]
        _SOLVED[(name, key)] = ({k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in sol.items()}, st)
    return _SOLVED[(name, key)]


def rho_of(sol, b, B):
    r = sol["rho"]
    if not torch.is_tensor(r):
        return torch.tensor([float(r)], dtype=torch.float64)
    r = r.double().reshape(-1)
    return r[b:b + 1] if r.numel() == B and B > 1 else r[:1]


@pytest.mark.parametrize("name", ROWS)
def test_status_and_iterations_are_the_tables(dev, monkeypatch, name):
    row = IT.ROWS[name]
    sol, st = solved(name, dev, monkeypatch, 'flag')
    assert sol["status"].dtype == torch.int32 and tuple(sol["status"].shape) == (row["B"],)
    print(name, "status", sol["status"].tolist(), "table", row["status"], "iters", sol["iters"].tolist(), "table", row["iters"], st)
    assert sol["status"].tolist() == row["status"]
    assert sol["iters"].tolist() == row["iters"]
    assert sol["iter"] == max(row["iters"]) == st["iters"]
    if name == "chunk_n20":
        assert st["mode_used"] == 2                      # (persistent, driven by the host in chunks)
    else:
        assert (st["loop_kind"], st["loop_workgroups_per_qp"]) == row["tier"]
    if row["m"] > 16 or row["dtype"] == torch.float64:
        assert st["linsolve_used"] == 1
    if name in ("split_n130_event", "big_n1030"):       # flagged BEHIND the event: the infeasible problems adapted rho
        assert st["n_factor"] >= 2
        given = row["control"]["rho"]
        assert all(float(rho_of(sol, b, row["B"])) != given for b in row["gross"] + row["mild"])


@pytest.mark.parametrize("name", ROWS)
def test_feasible_problems_keep_their_bits_and_flagged_ones_hold_the_iterate(dev, monkeypatch, name):
    row = IT.ROWS[name]
    B = row["B"]
    on, _ = solved(name, dev, monkeypatch, 'flag')
    off, _ = solved(name, dev, monkeypatch, None)
    own, t64 = IT.truth(name, row["dtype"]), IT.truth(name, torch.float64)
    bad = []
    for b in range(B):
        if row["status"][b] != IT.INFEASIBLE:
            for k in ("x", "u", "z", "lams", "nus"):
                if on[k] is not None and not H.same_bits(on[k][b], off[k][b]):
                    bad.append((b, k, "bits differ from the call without the key"))
            if not torch.equal(rho_of(on, b, B), rho_of(off, b, B)) or int(on["iters"][b]) != int(off["iters"][b]):
                bad.append((b, "rho / iters differ from the call without the key"))
            continue
        got = on["x"][b].double().reshape(-1)
        assert bool(torch.isfinite(on["x"][b]).all()) and bool(torch.isfinite(on["u"][b]).all())
        want, w64 = own[b]["x"].double().reshape(-1), t64[b]["x"].double().reshape(-1)
        scale = max(1.0, float(want.abs().max()))
        e_direct, e_hip64, e_ref64 = (float((a - c).abs().max()) for a, c in ((got, want), (got, w64), (want, w64)))
        print(name, b, "flagged x: direct", e_direct, "hip vs f64", e_hip64, "truth vs f64", e_ref64, "scale", scale)
        if row["dtype"] == torch.float64:
            ok = e_direct <= 1e-9 * scale
        else:
            ok = e_direct <= 1e-5 * scale or e_hip64 <= e_ref64 + 1e-5 * scale
        if not ok:
            bad.append((b, "x", dict(direct=e_direct, hip_vs_fp64=e_hip64, ref_vs_fp64=e_ref64, scale=scale)))
    assert not bad, bad


def test_without_the_key_an_infeasible_problem_runs_out_of_iterations(dev, monkeypatch):
    name = "split_n130"
    row = IT.ROWS[name]
    off, st = solved(name, dev, monkeypatch, None)
    last = row["control"]["max_iters"] - 1
    flagged = row["gross"] + row["mild"]
    print(name, "without the key", off["iters"].tolist(), st)
    assert [int(off["iters"][b]) for b in flagged] == [last] * len(flagged) and off["iter"] == last
    assert [int(off["iters"][b]) for b in range(row["B"]) if b not in flagged] == [row["iters"][b] for b in range(row["B"]) if b not in flagged]
    # ... and says so: 1 = ended at max_iters without being optimal, never 2
    assert off["status"].tolist() == [1 if b in flagged else 0 for b in range(row["B"])]


@pytest.mark.parametrize("name", ["small_n50", "split_n130"])
def test_raise_at_the_call_and_late(dev, name):
    row = IT.ROWS[name]
    flagged = sorted(row["gross"] + row["mild"])
    qp = gpu_inputs(row, dev)
    layer = L.SolveBoxQP(control=gpu_control(row, dev, infeasible='raise'))
    with pytest.raises(L.InfeasibleQPError) as err:
        layer(*qp)
    assert err.value.indices == flagged and isinstance(err.value, RuntimeError)
    # a call that does not wait: the error surfaces where the other late errors do
    L.synchronize()
    late = L.SolveBoxQP(control=gpu_control(row, dev, infeasible='raise', sync=False))
    x = late(*qp)
    assert tuple(x.shape) == (row["B"], row["n"], 1)
    with pytest.raises(L.InfeasibleQPError) as err:
        L.synchronize()
    assert err.value.indices == flagged
    L.synchronize()                                      # (raised once)
    # 'flag' never raises, and a batch without an infeasible problem does not either
    L.SolveBoxQP(control=gpu_control(row, dev, infeasible='flag'))(*qp)
    base = ET.ROWS["split_n130"]
    L.SolveBoxQP(control=L.box_qp_control(**dict(base["control"], stop='each', infeasible='raise')))(
        *(None if t is None else t.to(dev) for t in ET.inputs(base, base["dtype"])))
    L.synchronize()


@pytest.mark.parametrize("name", ["split_n130", "f64_n70_m3"])
def test_flag_zeroes_the_gradient_rows_of_flagged_problems(dev, name):
    row = IT.ROWS[name]
    B, n = row["B"], row["n"]
    flagged = sorted(row["gross"] + row["mild"])
    g = torch.Generator().manual_seed(7)
    cot = torch.randn(B, n, 1, generator=g, dtype=torch.float64).to(row["dtype"]).to(dev)

    def run(**extra):
        qp = [t.clone().requires_grad_(True) for t in gpu_inputs(row, dev)]
        x = L.SolveBoxQP(control=gpu_control(row, dev, **extra))(*qp)
        x.backward(cot)
        torch.cuda.synchronize()
        return x.detach(), dict(zip(GRADS, (qp[0].grad, qp[1].grad, qp[2].grad, qp[3].grad, qp[4].grad, qp[5].grad)))

    x_on, on = run(infeasible='flag')
    status = L.last_problem_status(dev)
    assert status.tolist() == row["status"]
    x_off, off = run()
    for k in GRADS:
        assert on[k] is not None, k
        for b in range(B):
            if b in flagged:
                assert int((on[k][b] != 0).sum()) == 0, (k, b, "a gradient row of a flagged problem is not zero")
            else:
                assert H.same_bits(on[k][b], off[k][b]), (k, b, "differs from the backward of the call without the key")
    assert all(H.same_bits(x_on[b], x_off[b]) for b in range(B) if b not in flagged)


@pytest.mark.parametrize("name", ["split_n130", "small_n100", "lu_n130_m17"])
def test_a_batch_without_an_infeasible_problem_is_untouched(dev, name):
    """rows of tests/each_table.py as they stand (small_n100: m = 0 with lb <= ub): no flag, every bit as without the key"""
    row = ET.ROWS[name]
    qp = tuple(None if t is None else t.to(dev) for t in ET.inputs(row, row["dtype"]))
    on = L.torch_solve_box_qp(*qp, L.box_qp_control(**dict(row["control"], stop='each', infeasible='flag')))
    on = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in on.items()}
    off = L.torch_solve_box_qp(*qp, L.box_qp_control(**dict(row["control"], stop='each')))
    assert on["status"].tolist() == [0] * row["B"] == off["status"].tolist()
    assert on["iters"].tolist() == row["iters"] == off["iters"].tolist() and on["iter"] == off["iter"]
    for k in ("x", "z", "u", "lams", "nus", "rho"):
        assert H.same_bits(on[k], off[k]), k


def test_a_batch_without_any_finite_bound_ignores_the_key(dev):
    row = ET.ROWS["split_n130"]
    Q, p, A, b, lb, ub = (None if t is None else t.to(dev) for t in ET.inputs(row, row["dtype"]))
    lb, ub = torch.full_like(lb, -float("inf")), torch.full_like(ub, float("inf"))
    on = L.torch_solve_box_qp(Q, p, A, b, lb, ub, L.box_qp_control(**dict(row["control"], stop='each', infeasible='flag')))
    on = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in on.items()}
    off = L.torch_solve_box_qp(Q, p, A, b, lb, ub, L.box_qp_control(**dict(row["control"], stop='each')))
    assert 2 not in on["status"].tolist() and on["status"].tolist() == off["status"].tolist()
    assert on["iters"].tolist() == off["iters"].tolist()
    for k in ("x", "nus"):
        assert H.same_bits(on[k], off[k]) and bool(torch.isfinite(on[k]).all()), k


MEM_ROW = "split_n130_event"          # the hot split loop, then the continuation kernel behind the event: the snapshot crosses a launch


def _mem_run(dev, monkeypatch, fill, keep=False):
    row = IT.ROWS[MEM_ROW]
    if not keep:
        H.release(_lib)
    with H.controlled_memory(monkeypatch, fill) as st:
        sol = L.torch_solve_box_qp(*(H.guarded(t) for t in gpu_inputs(row, dev)), gpu_control(row, dev, infeasible='flag'))
        torch.cuda.synchronize()
        counters = dict(created=st["ws_created"], reused=st["ws_reused"], grown=st["ws_grown"], unguarded=list(st["unguarded"]))
    found = dict(guards=H.check_guards(), inputs=H.check_inputs_untouched())
    out = {k: sol[k].detach().cpu().clone() for k in ("x", "u", "status", "iters")}
    return out, found, counters


@pytest.mark.parametrize("mode", ["00", "FF", "7F", "3C", "stale"])
def test_nothing_depends_on_what_the_enlarged_workspace_held(dev, monkeypatch, mode):
    """status, iters and x under a workspace (guards around it: the snapshots are its tail) and outputs that held 0x00 / 0xFF / 0x7F
    / 0x3C, or what a detecting solve of the same shape left behind -- marks and snapshots of exactly these checks included"""
    row = IT.ROWS[MEM_ROW]
    ref, found0, _ = _mem_run(dev, monkeypatch, 0x00)
    assert not found0["guards"] and not found0["inputs"], found0
    if mode == "stale":
        # what a run with another rho leaves: valid-looking marks at the same iterations
        with H.controlled_memory(monkeypatch, 0x00):
            L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row, dev, infeasible='flag', rho=100.))
            torch.cuda.synchronize()
        H.forget()
        out, found, counters = _mem_run(dev, monkeypatch, None, keep=True)
        assert counters["created"] == 0 and counters["reused"] >= 1, counters
    else:
        out, found, counters = _mem_run(dev, monkeypatch, H.FILLS[mode])
    H.release(_lib)
    print(MEM_ROW, mode, counters, out["status"].tolist(), out["iters"].tolist())
    assert out["status"].tolist() == row["status"] and out["iters"].tolist() == row["iters"]
    for k in ("x", "u", "status", "iters"):
        assert H.same_bits(out[k], ref[k]), k
    assert not found["guards"], found["guards"]
    assert not found["inputs"], found["inputs"]
    assert not counters["unguarded"], counters
