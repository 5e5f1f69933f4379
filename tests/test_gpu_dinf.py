"""control['unbounded'] on the GPU: every row of tests/dinf_table.py against its truth (solve_certify of each problem on its own).

For every row, with the key set: `status` and `iters` are the table's lists exactly (float32, float64 and the form of Qs x that does
not touch Q agree on them and every verdict stands clear of the threshold: tests/test_dinf_table.py), the row runs on the kernel
family it is named for, x of the optimal problems is the truth's at the bar of tests/test_gpu_each.py, and x of a flagged problem is
the truth's iterate of the detecting check at the same bar scaled by |x|_inf.  Then the layer: 'raise' (at the call, and late
through synchronize() when the call did not wait), 'flag' (gradient rows of flagged problems exactly zero, the others at the
gradient bar of tests/test_gpu_each.py), the key absent, control['infeasible'] alone, and that nothing depends on what the enlarged
workspace held.

Without the feature the key is ignored and the unbounded problems end at max_iters with status 1: every row-driven test here fails.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import infeas_table as IT
import dinf_table as DT
import memharness as H

pytestmark = pytest.mark.gpu

ROWS = list(DT.ROWS)
GRADS = ("dQ", "dp", "dA", "db", "dlb", "dub")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def keys_of(row, mode='flag'):
    """the row's keys: control['unbounded'], and control['infeasible'] too where the row holds a primal infeasible problem"""
    return dict(unbounded=mode, **(dict(infeasible=mode) if row["primal"] else {}))


def gpu_control(row, **extra):
    ctl = dict(row["control"], stop='each', **extra)
    if row["rho_b"] is not None and "rho" not in extra:
        ctl["rho"] = torch.tensor(row["rho_b"], dtype=row["dtype"], device="cuda:0").view(-1, 1, 1)
    ctl = L.box_qp_control(**ctl)
    ctl["check_solved"] = row["check"]      # (set on the dict: the factory files its argument under a key the solver never reads)
    return ctl


def schedule(monkeypatch, name):
    """the chunk row runs the host-driven persistent schedule, as tests/test_gpu_each.py reaches it"""
    if name == "chunk_n20":
        monkeypatch.setenv("LQP_SYNC_PLAN", "0")
        monkeypatch.setattr(SB, "_SYNC_SPLIT", False)


def gpu_inputs(row, dev):
    return tuple(None if t is None else t.to(dev) for t in DT.inputs(row, row["dtype"]))


_SOLVED = {}


def solved(name, dev, monkeypatch, on=True):
    """-> (solution on the host, last_forward_status) of the row with its keys set (on) or absent, computed once"""
    if (name, on) not in _SOLVED:
        row = DT.ROWS[name]
        schedule(monkeypatch, name)
        sol = L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row, **(keys_of(row) if on else {})))
        st = SB.last_forward_status(dev)
        assert L.last_problem_status(dev) is sol["status"]
        _SOLVED[(name, on)] = ({k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in sol.items()}, st)
    return _SOLVED[(name, on)]


def rho_of(sol, b, B):
    r = sol["rho"]
    if not torch.is_tensor(r):
        return torch.tensor([float(r)], dtype=torch.float64)
    r = r.double().reshape(-1)
    return r[b:b + 1] if r.numel() == B and B > 1 else r[:1]


@pytest.mark.parametrize("name", ROWS)
def test_status_and_iterations_are_the_tables(dev, monkeypatch, name):
    row = DT.ROWS[name]
    sol, st = solved(name, dev, monkeypatch)
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
    if name in ("split_n130_event", "big_n1030"):       # flagged BEHIND the event: the unbounded problems adapted rho
        assert st["n_factor"] >= 2
        given = row["control"]["rho"]
        assert all(float(rho_of(sol, b, row["B"])) != given for b in row["gross"] + row["mild"])


@pytest.mark.parametrize("name", ROWS)
def test_x_is_the_truths_for_optimal_and_for_flagged_problems(dev, monkeypatch, name):
    row = DT.ROWS[name]
    sol, _ = solved(name, dev, monkeypatch)
    own, t64 = DT.truth(name, row["dtype"]), DT.truth(name, torch.float64)
    bad = []
    for b in range(row["B"]):
        got = sol["x"][b].double().reshape(-1)
        assert bool(torch.isfinite(sol["x"][b]).all()) and bool(torch.isfinite(sol["u"][b]).all())
        want, w64 = own[b]["x"].double().reshape(-1), t64[b]["x"].double().reshape(-1)
        scale = max(1.0, float(want.abs().max()))        # (a flagged problem: the bar scaled by |x|_inf of the detecting check)
        e_direct, e_hip64, e_ref64 = (float((a - c).abs().max()) for a, c in ((got, want), (got, w64), (want, w64)))
        print(name, b, "status", row["status"][b], "x: direct", e_direct, "hip vs f64", e_hip64, "truth vs f64", e_ref64, "scale", scale)
        if row["dtype"] == torch.float64:
            ok = e_direct <= 1e-9 * scale
        else:
            ok = e_direct <= 1e-5 * scale or e_hip64 <= e_ref64 + 1e-5 * scale
        if not ok:
            bad.append((b, row["status"][b], dict(direct=e_direct, hip_vs_fp64=e_hip64, ref_vs_fp64=e_ref64, scale=scale)))
    assert not bad, bad


def test_key_absent_is_the_call_that_never_had_it_and_runs_out_of_iterations(dev, monkeypatch):
    name = "split_n130"
    row = DT.ROWS[name]
    off, st = solved(name, dev, monkeypatch, on=False)
    last = row["control"]["max_iters"] - 1
    flagged = row["gross"] + row["mild"]
    print(name, "without the key", off["status"].tolist(), off["iters"].tolist(), st)
    assert off["status"].tolist() == [1 if b in flagged else 0 for b in range(row["B"])]
    assert [int(off["iters"][b]) for b in flagged] == [last] * len(flagged) and off["iter"] == last
    assert [int(off["iters"][b]) for b in range(row["B"]) if b not in flagged] == [row["iters"][b] for b in range(row["B"]) if b not in flagged]
    # the key present and None, and a threshold without its key: the same call, bit for bit
    for extra in (dict(unbounded=None), dict(eps_dual_inf=1e-3), dict(unbounded=None, infeasible=None)):
        same = L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row, **extra))
        assert same["status"].tolist() == off["status"].tolist() and same["iters"].tolist() == off["iters"].tolist()
        for k in ("x", "z", "u", "lams", "nus"):
            assert H.same_bits(same[k].cpu(), off[k]), (extra, k)
    # ... and with the key, every problem that is not flagged keeps the bits of the call without it
    on, _ = solved(name, dev, monkeypatch)
    for b in range(row["B"]):
        if b not in flagged:
            assert all(H.same_bits(on[k][b], off[k][b]) for k in ("x", "z", "u", "lams", "nus")), b


@pytest.mark.parametrize("name", ["small_n50", "split_n130", "mixed_n130"])
def test_raise_at_the_call_and_late(dev, name):
    row = DT.ROWS[name]
    flagged = sorted(row["gross"] + row["mild"])
    qp = gpu_inputs(row, dev)
    keys = dict(unbounded='raise', **(dict(infeasible='flag') if row["primal"] else {}))
    layer = L.SolveBoxQP(control=gpu_control(row, **keys))
    with pytest.raises(L.UnboundedQPError) as err:
        layer(*qp)
    assert err.value.indices == flagged and isinstance(err.value, RuntimeError) and not isinstance(err.value, L.InfeasibleQPError)
    # a call that does not wait: the error surfaces where the other late errors do
    L.synchronize()
    late = L.SolveBoxQP(control=gpu_control(row, sync=False, **keys))
    x = late(*qp)
    assert tuple(x.shape) == (row["B"], row["n"], 1)
    with pytest.raises(L.UnboundedQPError) as err:
        L.synchronize()
    assert err.value.indices == flagged
    L.synchronize()                                      # (raised once)
    if row["primal"]:                                    # both 'raise': the primal error comes first
        with pytest.raises(L.InfeasibleQPError) as err:
            L.SolveBoxQP(control=gpu_control(row, unbounded='raise', infeasible='raise'))(*qp)
        assert err.value.indices == sorted(row["primal"])
    # 'flag' never raises
    L.SolveBoxQP(control=gpu_control(row, **keys_of(row)))(*qp)
    L.synchronize()


def oracle_grads(name, dtype, cot, problems):
    """the oracle's fixed-point backward on the truth's solution of every problem in `problems` -> six lists"""
    row = DT.ROWS[name]
    sols, q = DT.truth(name, dtype), DT.inputs(row, dtype)
    out = [[] for _ in range(6)]
    for b in problems:
        s, one = sols[b], tuple(t[b:b + 1] for t in q)
        gr = O.solve_box_qp_grad(cot[b:b + 1].to(dtype), s["x"], s["u"], s["lams"], s["nus"], one[0], one[2], one[4], one[5], s["rho"])
        for k in range(6):
            out[k].append(gr[k].double())
    return out


@pytest.mark.parametrize("name", ["split_n130", "f64_n70_m3", "mixed_n130"])
def test_flag_zeroes_the_gradient_rows_of_flagged_problems(dev, name):
    row = DT.ROWS[name]
    B, n = row["B"], row["n"]
    f64 = row["dtype"] == torch.float64
    flagged = sorted(row["gross"] + row["mild"] + row["primal"])
    rest = [b for b in range(B) if b not in flagged]
    cot = torch.randn(B, n, 1, generator=torch.Generator().manual_seed(7), dtype=torch.float64).to(row["dtype"])
    qp = [t.clone().requires_grad_(True) for t in gpu_inputs(row, dev)]
    x = L.SolveBoxQP(control=gpu_control(row, **keys_of(row)))(*qp)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    assert L.last_problem_status(dev).tolist() == row["status"]
    got = [t.grad for t in qp]
    own, t64 = oracle_grads(name, row["dtype"], cot, rest), oracle_grads(name, torch.float64, cot, rest)
    rtol = 1e-6 if f64 else 1e-4
    for k, nm in enumerate(GRADS):
        assert got[k] is not None, nm
        for b in flagged:
            assert int((got[k][b] != 0).sum()) == 0, (nm, b, "a gradient row of a flagged problem is not zero")
        scale = max(float(o.abs().max()) for o in own[k])
        for j, b in enumerate(rest):
            g = got[k][b:b + 1].cpu().double()
            e_direct, e_hip64, e_ref64 = (float((a - c).abs().max()) for a, c in ((g, own[k][j]), (g, t64[k][j]), (own[k][j], t64[k][j])))
            print(name, nm, b, dict(direct=e_direct, hip_vs_fp64=e_hip64, ref_vs_fp64=e_ref64, scale=scale))
            assert bool(torch.isfinite(g).all())
            assert e_direct <= rtol * scale or (not f64 and e_hip64 <= e_ref64 + rtol * scale), (nm, b, e_direct, e_hip64, e_ref64, scale)


def test_infeasible_alone_is_what_it_was(dev):
    """control['infeasible'] without the new key, through the same kernels: a row of tests/infeas_table.py, its statuses and iterations"""
    row = IT.ROWS["split_n130"]
    qp = tuple(None if t is None else t.to(dev) for t in IT.inputs(row, row["dtype"]))
    sol = L.torch_solve_box_qp(*qp, L.box_qp_control(**dict(row["control"], stop='each', infeasible='flag')))
    st = SB.last_forward_status(dev)
    print("infeas_table split_n130", sol["status"].tolist(), sol["iters"].tolist(), st)
    assert sol["status"].tolist() == row["status"] and sol["iters"].tolist() == row["iters"]
    assert (st["loop_kind"], st["loop_workgroups_per_qp"]) == row["tier"]
    # ... and with the new key on top no problem of it is flagged unbounded: every bound is finite
    both = L.torch_solve_box_qp(*qp, L.box_qp_control(**dict(row["control"], stop='each', infeasible='flag', unbounded='flag')))
    assert both["status"].tolist() == row["status"] and both["iters"].tolist() == row["iters"]
    for k in ("x", "u", "nus"):
        assert H.same_bits(both[k], sol[k]), k


MEM_ROW = "split_n130_event"          # the hot split loop, then the continuation kernel behind the event: the snapshot crosses a launch


def _mem_run(dev, monkeypatch, fill, keep=False):
    row = DT.ROWS[MEM_ROW]
    if not keep:
        H.release(_lib)
    with H.controlled_memory(monkeypatch, fill) as st:
        sol = L.torch_solve_box_qp(*(H.guarded(t) for t in gpu_inputs(row, dev)), gpu_control(row, **keys_of(row)))
        torch.cuda.synchronize()
        counters = dict(created=st["ws_created"], reused=st["ws_reused"], grown=st["ws_grown"], unguarded=list(st["unguarded"]))
    found = dict(guards=H.check_guards(), inputs=H.check_inputs_untouched())
    out = {k: sol[k].detach().cpu().clone() for k in ("x", "u", "status", "iters")}
    return out, found, counters


@pytest.mark.parametrize("mode", ["FF", "stale"])
def test_nothing_depends_on_what_the_enlarged_workspace_held(dev, monkeypatch, mode):
    """status, iters and x under a workspace (guards around it: the snapshots with x and Qs x are its tail) and outputs that held
    0xFF, or what a certifying solve of the same shape left behind -- marks and snapshots of exactly these checks included"""
    row = DT.ROWS[MEM_ROW]
    ref, found0, _ = _mem_run(dev, monkeypatch, 0x00)
    assert not found0["guards"] and not found0["inputs"], found0
    if mode == "stale":
        # what a run with another rho leaves: valid-looking marks at the same iterations
        with H.controlled_memory(monkeypatch, 0x00):
            L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row, rho=100., **keys_of(row)))
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
