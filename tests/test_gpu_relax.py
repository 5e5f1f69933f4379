"""control['alpha'] on the GPU: every row of tests/relax_table.py against the relaxed truth at a pinned iteration count, solves that
stop by themselves a third earlier, alpha = 1.0 against the key absent bit for bit, and gradients through the module.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= 4 |t32 - t64| + 1e-7 scale, float64 1e-9 scale, t32 / t64
the relaxed truth in float32 / float64.  tests/test_relax_table.py shows, without a GPU, that the plain step misses every row's bar
by at least 100 x: all of these fail on a library that ignores the key.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import each_table as E
import relax_table as RT
import tier_table as T

pytestmark = pytest.mark.gpu
HIP_KEYS = ("linsolve", "launch_mode")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _control(r, **extra):
    return O.make_control(**T.control(r), **{k: r["ctl"][k] for k in HIP_KEYS if k in r["ctl"]}, **extra)


def _pick(v, idx):
    if torch.is_tensor(v) and v.dim() > 0:
        return v[torch.tensor(idx).to(v.device)].detach().cpu()
    return v


def _report(what, res):
    for k, rec in res.items():
        print(what, k, "err %.3e" % rec["err"], "bar %.3e" % rec["bar"], "ratio", rec.get("ratio"))


@pytest.mark.parametrize("key", list(RT.ROWS))
def test_row_against_the_relaxed_truth(dev, cus, monkeypatch, key):
    r = RT.ROWS[key]
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in T.inputs(r, B)]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    sol = L.torch_solve_box_qp(*args, _control(r, alpha=r["alpha"]))
    st, bad = sol["_stats"], []
    if r["ctl"].get("sync", True) is False:
        # the module's un-synchronised path: the same schedule, enqueued whole; nothing reports back but the device's status block
        x = L.SolveBoxQP(control=_control(r, alpha=r["alpha"], sync=False))(*args)
        mst = SB.last_forward_status(dev)
        if mst["iters"] != r["K"] or not torch.equal(x, sol["x"]):
            bad.append(("sync=False", mst["iters"], bool(torch.equal(x, sol["x"]))))
    idx, t32, t64 = RT.row_truth(key, cus)
    if sol["iter"] != r["K"]:
        bad.append(("iter", sol["iter"], r["K"]))
    bad += [("sig", k, st[k], v) for k, v in r["sig"].items() if st[k] != v]
    if st["n_factor"] != t64["n_factor"] or (t32 is not None and t32["n_factor"] != t64["n_factor"]):
        bad.append(("n_factor", st["n_factor"], t64["n_factor"]))
    res = T.compare(r, {k: _pick(sol[k], idx) for k in T.OUTPUTS}, t32, t64)
    _report(key, res)
    bad += [("value", k, rec) for k, rec in res.items() if not rec["ok"]]
    assert not bad, (key, bad)


@pytest.mark.parametrize("case", list(RT.STOPS))
def test_a_relaxed_solve_stops_earlier(dev, case):
    n, B, seed = case
    plain, relaxed = RT.STOPS[case]
    args = [t.to(dev) for t in O.create_qp_data(n, B, seed=seed)]
    sol1 = L.torch_solve_box_qp(*args, O.make_control(**RT.STOP_CONTROL))
    sola = L.torch_solve_box_qp(*args, O.make_control(**RT.STOP_CONTROL, alpha=RT.ALPHA))
    print(case, "iter", sol1["iter"], sola["iter"])
    assert sol1["iter"] == plain and sola["iter"] == relaxed
    t32, t64 = (RT.stop_truth(n, B, seed, RT.ALPHA, dt) for dt in (torch.float32, torch.float64))
    res = T.compare(RT.STOP_ROW, {k: _pick(sola[k], list(range(B))) for k in T.OUTPUTS}, t32, t64, keys=("x",))
    _report(case, res)
    assert res["x"]["ok"], res


@pytest.mark.parametrize("name", RT.SAME_BITS)
def test_alpha_one_is_the_key_absent_bit_for_bit(dev, cus, monkeypatch, name):
    r = T.ROW_BY_NAME[name]
    args = [None if t is None else t.to(dev) for t in T.inputs(r, T.batch(r, cus))]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    absent = L.torch_solve_box_qp(*args, _control(r))
    one = L.torch_solve_box_qp(*args, _control(r, alpha=1.0))
    assert absent["iter"] == one["iter"] == r["K"]
    assert all(absent["_stats"][k] == v for k, v in r["sig"].items()), absent["_stats"]
    for k in T.OUTPUTS:
        a, b = absent[k], one[k]
        assert (a is None and b is None) or (torch.equal(a, b) if torch.is_tensor(a) else a == b), k


def test_each_problem_stops_at_its_own_relaxed_count(dev):
    """stop = 'each' on the split loop: every problem of the each-table's row against ITS relaxed solve as a batch of one"""
    row = E.ROWS[RT.EACH_ROW]
    B = row["B"]
    args = [None if t is None else t.to(dev) for t in E.inputs(row, row["dtype"])]
    sol = L.torch_solve_box_qp(*args, L.box_qp_control(**dict(row["control"], stop='each', alpha=RT.ALPHA)))
    s32, s64 = RT.each_truth(torch.float32), RT.each_truth(torch.float64)
    want = [s["iter"] for s in s64]
    got = sol["iters"].cpu().tolist()
    print(RT.EACH_ROW, "iterations per problem", got, "relaxed truth", want, "plain", row["iters"])
    assert got == want and sol["iter"] == max(want)
    assert SB.last_forward_status(dev)["loop_workgroups_per_qp"] == 2
    bad = []
    for b in range(B):
        hip = {k: (None if sol[k] is None else sol[k][b:b + 1].detach().cpu()) for k in ("x", "z", "u", "lams", "nus")}
        hip["rho"] = sol["rho"][b:b + 1].detach().cpu() if torch.is_tensor(sol["rho"]) and sol["rho"].numel() == B else sol["rho"]
        res = T.compare(RT.STOP_ROW, hip, s32[b], s64[b])
        bad += [(b, k, rec) for k, rec in res.items() if not rec["ok"]]
    assert not bad, bad


@pytest.mark.parametrize("name", list(RT.GRAD_ROWS))
@pytest.mark.parametrize("backward", ["fixed_point", "kkt"])
def test_gradients_through_a_relaxed_forward(dev, cus, name, backward):
    r = RT.GRAD_ROWS[name]
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in T.inputs(r, B)]
    leaves = [None if (t is None or i > 3) else t.clone().requires_grad_(True) for i, t in enumerate(args)]
    cot = RT.cot_of(r, B, args[1].dtype)
    x = L.SolveBoxQP(control=_control(r, alpha=r["alpha"], backward=backward))(*leaves[:4], args[4], args[5])
    mst = SB.last_forward_status(dev)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    assert mst["iters"] == r["K"] and all(mst[{"loop_workgroups": "loop_workgroups_per_qp"}.get(k, k)] == v for k, v in r["sig"].items()
                                          if k != "factor_launches"), mst
    idx, t32, t64 = RT.row_truth(name, cus, "GRAD_ROWS")
    sub = T.inputs(r, B, idx)
    g32 = RT.truth_grads(r, sub, t32, cot[idx], torch.float32, backward)
    g64 = RT.truth_grads(r, sub, t64, cot[idx], torch.float64, backward)
    res = T.compare(r, {k: _pick(t.grad, idx) for k, t in zip(T.GRADS, leaves)}, g32, g64, keys=T.GRADS)
    res.update(T.compare(r, {"x": _pick(x, idx)}, t32, t64, keys=("x",)))
    _report(f"{name} {backward}", res)
    bad = [(k, rec) for k, rec in res.items() if not rec["ok"]]
    assert not bad, (name, backward, bad)
