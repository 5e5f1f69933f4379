"""control['stop'] = 'each' on the GPU: every row of tests/each_table.py against the oracle's solve of each problem on its own.

For every row: the per-problem iteration counts are the table's (the float32 and float64 oracles agree on them: tests/
test_each_table.py), sol['iter'] is their maximum, and x, z, u, lams, nus, rho of every problem are its solo oracle's at the project's
bar -- float32 within 1e-5 of the scale, or no further from the float64 solo solve than the oracle's own float32 one (+ 1e-5), the
criterion of tests/test_gpu_parity.py (close_or_fp64); float64 within 1e-9.  Every row asserts the tier it is named for through
last_forward_status (`loop_kind`, `loop_workgroups_per_qp`): the small loop, the split loop on two / four
workgroups per problem, the one-workgroup loop where a switch, the launch mode or the x-update asks for it.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import each_table as ET
import kkt_table as KT
import tier_table as T

pytestmark = pytest.mark.gpu

KEYS = ("x", "z", "u", "lams", "nus", "rho")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def gpu_control(row, **extra):
    return L.box_qp_control(**dict(row["control"], stop='each', **extra))


def gpu_inputs(row, dev, sl=slice(None)):
    return tuple(None if t is None else t[sl].to(dev) for t in ET.inputs(row, row["dtype"]))


def as_rho(rho, b, B):
    """the rho of problem b, whatever form it came back in: a number (given and never adapted), (B,1,1) or (1,1,1)"""
    if not torch.is_tensor(rho):
        return torch.tensor([float(rho)], dtype=torch.float64)
    r = rho.detach().cpu().double().reshape(-1)
    return r[b:b + 1] if r.numel() == B and B > 1 else r[:1]


def part(sol, k, b, B):
    if k == "rho":
        return as_rho(sol["rho"], b, B)
    t = sol[k]
    return None if t is None else t[b].detach().cpu().double().reshape(-1)


def compare(name, sol, problems=None, what=KEYS):
    """every problem's outputs against its solo oracle; -> the list of failures"""
    row = ET.ROWS[name]
    f64 = row["dtype"] == torch.float64
    s_own, s64 = ET.solo(name, row["dtype"]), ET.solo(name, torch.float64)
    problems = list(range(row["B"])) if problems is None else problems
    bad = []
    for j, b in enumerate(problems):
        for k in what:
            got, own, t64 = part(sol, k, j, len(problems)), part(s_own[b], k, 0, 1), part(s64[b], k, 0, 1)
            if own is None:
                assert got is None
                continue
            scale = max(1.0, float(own.abs().max()))
            e_direct = float((got - own).abs().max())
            if f64:
                ok, fig = e_direct <= 1e-9 * scale, dict(direct=e_direct, tol=1e-9 * scale)
            else:
                e_hip64, e_ref64 = float((got - t64).abs().max()), float((own - t64).abs().max())
                ok = e_direct <= 1e-5 * scale or e_hip64 <= e_ref64 + 1e-5 * scale
                fig = dict(direct=e_direct, hip_vs_fp64=e_hip64, ref_vs_fp64=e_ref64, tol=1e-5 * scale)
            if not ok:
                bad.append((name, b, k, fig))
    return bad


def check_solution(name, sol, problems=None):
    row = ET.ROWS[name]
    want = row["iters"] if problems is None else [row["iters"][b] for b in problems]
    assert sol["iters"].dtype == torch.int32 and sol["iters"].is_cuda and tuple(sol["iters"].shape) == (len(want),)
    got = sol["iters"].cpu().tolist()
    print(name, "iterations per problem", got, "table", want)
    assert got == want
    assert isinstance(sol["iter"], int) and sol["iter"] == max(want)
    bad = compare(name, sol, problems)
    assert not bad, bad


# (row, extra control keys, environment switches, workgroups per problem of the loop or None)
CASES = [
    ("small_n100", {}, {}, "small"),
    ("small_n100", {}, {"LQP_LOOP_SMALL": "0"}, 1),
    ("small_n50_event", {}, {}, "small"),
    ("split_n130", {}, {}, 2),
    ("split_n449", {}, {}, 4),
    ("split_n449", {}, {"LQP_LOOP_SPLIT4": "0"}, 2),
    ("split_n130_event", {}, {}, 2),
    ("split_n130", {}, {"LQP_LOOP_SPLIT": "0"}, 1),
    ("split_n130_event", {}, {"LQP_LOOP_SPLIT": "0"}, 1),
    ("split_n130", {"launch_mode": 1}, {}, 1),
    ("split_n130_event", {"launch_mode": 1}, {}, 1),
    ("split_n130", {"launch_mode": 2}, {}, 2),
    ("split_n130", {"linsolve": "lu"}, {}, 1),
    ("split_n130", {"linsolve": "spd"}, {}, 2),
    ("lu_n130_m17", {}, {}, 1),
    ("f64_n70_m3", {}, {}, 1),
    ("f64_n70_m3_event", {}, {}, 1),
    ("f64_n70_m3_event", {"launch_mode": 1}, {}, 1),
    ("big_n1030", {}, {}, 1),
]



@pytest.mark.parametrize("name,extra,env,wg", CASES, ids=[f"{c[0]}-{'-'.join(f'{k}{v}' for k, v in {**c[1], **c[2]}.items()) or 'default'}" for c in CASES])
def test_every_problem_is_solved_as_a_batch_of_one(dev, monkeypatch, name, extra, env, wg):
    row = ET.ROWS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sol = L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row, **extra))
    check_solution(name, sol)
    st = SB.last_forward_status(dev)
    print(name, extra, env, st)
    assert st["iters"] == max(row["iters"])
    # the tier the row is named for: workgroups per problem of the loop, and its kernel family (0 one workgroup, 1 split, 2 small)
    assert st["loop_workgroups_per_qp"] == (1 if wg == "small" else wg)
    assert st["loop_kind"] == (2 if wg == "small" else 1 if wg in (2, 4) else 0)
    if wg == "small" or (wg in (2, 4) and "launch_mode" not in extra):
        assert st["mode_used"] in (2, 4)
    if extra.get("linsolve") == "lu" or row["m"] > 16 or row["dtype"] == torch.float64:
        assert st["linsolve_used"] == 1
    if extra.get("linsolve") == "spd":
        assert st["linsolve_used"] == 2
    if row["adapts"] is not None:
        assert sol["_stats"]["rho_updated"] == 1 and st["n_factor"] >= 2
        # who adapted: the rho that came back differs from the given one exactly for those problems
        rho = sol["rho"].cpu().reshape(-1)
        assert [bool(r != row["control"]["rho"]) for r in rho.tolist()] == row["adapts"]
    else:
        assert st["n_factor"] == 1


def test_host_driven_persistent_chunks(dev, monkeypatch):
    """The persistent loop driven by the host in chunks (a C caller that lets the library wait; more adaptive-rho events than the
    up-front schedule takes): every chunk ends in k_check_done on its last check.  A problem that is still running there must keep the
    batch going: one stops behind the first chunk boundary (512 iterations at a check every iteration), two run to max_iters - 1."""
    name = "chunk_n20"
    row = ET.ROWS[name]
    monkeypatch.setenv("LQP_SYNC_PLAN", "0")
    monkeypatch.setattr(SB, "_SYNC_SPLIT", False)
    _lib.profile(enable=True, reset=True)
    try:
        sol = L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row))
        torch.cuda.synchronize()
        used = _lib.profile()
    finally:
        _lib.profile(enable=False)
    st = SB.last_forward_status(dev)
    print(name, st, {k: v[1] for k, v in used.items() if v[1]})
    assert st["mode_used"] == 2 and used["misc"][1] >= 2          # (persistent, and k_check_done behind each of its chunks)
    got = sol["iters"].cpu().tolist()
    print(name, "iterations per problem", got, "table", row["iters"])
    assert got == row["iters"] and sol["iter"] == row["control"]["max_iters"] - 1
    done = [b for b in range(row["B"]) if b not in row["never"]]
    bad = compare(name, {k: (sol[k] if not torch.is_tensor(sol[k]) else sol[k][done]) for k in ("x", "z", "u", "lams", "nus")},
                  problems=done, what=("x", "z", "u", "lams", "nus"))
    assert not bad, bad


def test_default_is_untouched(dev):
    """stop='all' and no key at all: identical bits, no 'iters' -- and not the solo results (the early problems iterate on)"""
    row = ET.ROWS["split_n130"]
    qp = gpu_inputs(row, dev)
    a = L.torch_solve_box_qp(*qp, L.box_qp_control(**row["control"]))
    b = L.torch_solve_box_qp(*qp, L.box_qp_control(**dict(row["control"], stop='all')))
    assert "iters" not in a and "iters" not in b
    assert a["iter"] == b["iter"] == max(row["iters"])
    for k in ("x", "z", "u", "lams", "nus"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["rho"], b["rho"])
    each = L.torch_solve_box_qp(*qp, gpu_control(row))
    moved = [not torch.equal(each["x"][i], a["x"][i]) for i in range(row["B"]) if 0 < row["iters"][i] < max(row["iters"])]
    assert len(moved) >= 3 and all(moved)


def test_results_do_not_depend_on_the_batch(dev):
    """the property the mode is for: eight problems as one batch, and as two batches of four"""
    name = "split_n130"
    row = ET.ROWS[name]
    whole = L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row))
    whole = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in whole.items()}
    for lo in (0, 4):
        half = L.torch_solve_box_qp(*gpu_inputs(row, dev, slice(lo, lo + 4)), gpu_control(row))
        check_solution(name, half, problems=list(range(lo, lo + 4)))
        assert torch.equal(half["iters"], whole["iters"][lo:lo + 4])
        scale = max(1.0, float(whole["x"].abs().max()))
        assert float((half["x"] - whole["x"][lo:lo + 4]).abs().max()) <= 1e-5 * scale


def test_turn_taking_segments(dev):
    """More problems than half the CUs: the split loop per check segment, its pairs taking turns on the chip.  The split row's eight
    problems, twenty times over: every copy stops where its original does alone, with the original's iterate."""
    name = "split_n130"
    row = ET.ROWS[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = cus // (2 * row["B"]) + 4           # (2 B > #CUs, with room)
    qp = tuple(None if t is None else t.repeat(reps, *([1] * (t.dim() - 1))) for t in gpu_inputs(row, dev))
    sol = L.torch_solve_box_qp(*qp, gpu_control(row))
    st = SB.last_forward_status(dev)
    print(name, "x", reps, st)
    assert st["loop_workgroups_per_qp"] == 2 and st["mode_used"] == 1
    assert sol["iters"].cpu().tolist() == row["iters"] * reps and sol["iter"] == max(row["iters"])
    for r in (0, reps // 2, reps - 1):
        sl = slice(r * row["B"], (r + 1) * row["B"])
        bad = compare(name, {k: (None if sol[k] is None else sol[k][sl]) for k in ("x", "z", "u", "lams", "nus")}, what=("x", "z", "u", "lams", "nus"))
        assert not bad, (r, bad)


def test_pipelined_call(dev):
    """sync=False: nothing waits; the results once the stream is through, and no error reported late"""
    name = "split_n130"
    row = ET.ROWS[name]
    sol = SB._forward_solve(*gpu_inputs(row, dev), gpu_control(row), sync=False)
    assert sol["_stats"]["mode_used"] == 3 and "iters" in sol
    L.synchronize()
    got = sol["iters"].cpu().tolist()
    assert got == row["iters"]
    bad = compare(name, sol)
    assert not bad, bad
    st = SB.last_forward_status(dev)
    assert st["iters"] == max(row["iters"]) and st["loop_workgroups_per_qp"] == 2
    L.synchronize()


def test_verbose_trace_is_the_maximum_over_the_running_problems(dev, capsys):
    name = "small_n100"
    row = ET.ROWS[name]
    sol = L.torch_solve_box_qp(*gpu_inputs(row, dev), gpu_control(row, verbose=True))
    assert sol["iters"].cpu().tolist() == row["iters"]
    lines = capsys.readouterr().out.splitlines()
    its = [int(ln.split("=")[1]) for ln in lines if ln.startswith("iteration")]
    assert its == list(range(0, max(row["iters"]) + 1, 10))
    # the last check was held by the slowest problem alone: its own errors, which the solo oracle prints too
    pri = [float(ln.split("=")[1]) for ln in lines if "primal_error" in ln]
    assert len(pri) == len(its) and all(p >= 0.0 for p in pri) and pri[-1] < pri[0]


@pytest.mark.parametrize("name,backward", [("split_n130", "fixed_point"), ("f64_n70_m3", "fixed_point"), ("split_n130", "kkt")])
def test_backward_through_the_module(dev, monkeypatch, name, backward):
    """x.backward(cot) behind a stop='each' forward: all six gradients against the oracle's fixed-point backward on the SOLO
    solutions (rtol 1e-4 of the gradient's scale, 1e-6 in float64); the prefactored and the one-call backward give the same bits"""
    row = ET.ROWS[name]
    f64 = row["dtype"] == torch.float64
    B, n = row["B"], row["n"]
    cot = torch.randn(B, n, 1, generator=torch.Generator().manual_seed(7), dtype=torch.float64).to(row["dtype"])
    qp = ET.inputs(row, row["dtype"])

    def run(prefactor):
        monkeypatch.setattr(SB, "_PREFACTOR_BWD", prefactor)
        leaves = [t.clone().to(dev).requires_grad_(True) for t in qp]
        x = L.SolveBoxQP(control=gpu_control(row, backward=backward))(*leaves)
        x.backward(cot.to(dev))
        torch.cuda.synchronize()
        return x.detach(), [t.grad for t in leaves]

    x1, g1 = run(True)
    x0, g0 = run(False)
    assert torch.equal(x0, x1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    bad = compare(name, {"x": x1}, what=("x",))
    assert not bad, bad
    fwd = L.torch_solve_box_qp(*(t.to(dev) for t in qp), gpu_control(row))      # (the same forward again: its duals)
    assert torch.equal(fwd["x"], x1)

    def oracle_grads(dtype):
        solo, q = ET.solo(name, dtype), ET.inputs(row, dtype)
        out = [[] for _ in range(6)]
        for b in range(B):
            s, one = solo[b], tuple(t[b:b + 1] for t in q)
            if backward == "kkt":
                gr = O.solve_box_qp_grad_kkt(cot[b:b + 1].to(dtype), s["x"], s["lams"], s["nus"], one[0], one[2], one[4], one[5])
            else:
                gr = O.solve_box_qp_grad(cot[b:b + 1].to(dtype), s["x"], s["u"], s["lams"], s["nus"], one[0], one[2], one[4], one[5], s["rho"])
            for k in range(6):
                out[k].append(gr[k])
        return [torch.cat(o, 0).double() for o in out]

    own, t64 = oracle_grads(row["dtype"]), oracle_grads(torch.float64)
    rtol = 1e-6 if f64 else 1e-4
    for k, nm in enumerate(("dQ", "dp", "dA", "db", "dlb", "dub")):
        if backward == "kkt" and nm in ("dlb", "dub"):
            # The KKT form divides the dx of a variable at its bound by its slack floor, 1e-8: the 1e-5 by which the forward differs from
            # its oracle is not comparable through that.  These two are held to the budget of tests/kkt_table.py instead, on ONE point:
            # the oracle's KKT backward of the GPU forward's own (x, lams, nus) -- |hip - t64| <= R |t32 - t64| + F scale, its defaults
            pt = (cot, fwd["x"].cpu(), fwd["lams"].cpu(), fwd["nus"].cpu(), qp[0], qp[2], qp[4], qp[5])
            t32k, t64k = KT.oracle(pt, torch.float32), KT.oracle(pt, torch.float64)
            rec = T.compare(dict(dtype="f32", R=T.R_DEFAULT, F=T.F_DEFAULT), {nm: g1[k].cpu()}, t32k, t64k, keys=(nm,))[nm]
            print(name, nm, rec)
            assert rec["ok"], (nm, rec)
            continue
        got, scale = g1[k].cpu().double(), float(own[k].abs().max())
        e_direct, e_hip64, e_ref64 = (float((a - b).abs().max()) for a, b in ((got, own[k]), (got, t64[k]), (own[k], t64[k])))
        print(name, nm, dict(direct=e_direct, hip_vs_fp64=e_hip64, ref_vs_fp64=e_ref64, scale=scale))
        assert e_direct <= rtol * scale or (not f64 and e_hip64 <= e_ref64 + rtol * scale), (nm, e_direct, e_hip64, e_ref64, scale)
