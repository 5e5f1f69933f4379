"""The L1 layer on the GPU: every row of tests/l1_table.py against its truth at a pinned iteration count, w = 0 against the plain
forward bit for bit, all eight gradients through the module, a solve that stops by itself, and a memory row.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale, t32 / t64 the
truth (l1_table.solve_l1) in float32 / float64.  `side` is compared exactly; an element may differ only where the float64 truth
says it sits within the bar for z of changing its set (l1_table.excused), and at most 1 % of a problem's elements may.
tests/test_l1_table.py shows, without a GPU, that the unthresholded iterates miss every row's bar by at least 100 x.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import l1_table as LT
import tier_table as T

pytestmark = pytest.mark.gpu
HIP_KEYS = ("linsolve", "launch_mode")
VALUES = tuple(k for k in LT.OUTPUTS if k != "side")
# (the gradients' bars are the ones tests/test_gpu_fp.py uses, fp_table.compare: tier_table.compare over every gradient; dw and dc
#  take them like dp and dlb)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _control(r, **extra):
    c = O.make_control(**T.control(r), **{k: r["ctl"][k] for k in HIP_KEYS if k in r["ctl"]}, **extra)
    if r.get("alpha", 1.0) != 1.0:
        c["alpha"] = r["alpha"]
    return c


def _pick(v, idx):
    if torch.is_tensor(v) and v.dim() > 0:
        return v[torch.tensor(idx).to(v.device)].detach().cpu()
    return v


def _report(what, res):
    for k, rec in res.items():
        print(what, k, "err %.3e" % rec["err"], "bar %.3e" % rec["bar"], "ratio", rec.get("ratio"))


def _side_check(what, side, t64, bar_z):
    """-> list of failures: `side` against the float64 truth's, exact outside the margin, at most 1 % of a problem inside it"""
    bad = []
    diff = side.double() != t64["side"]
    ok = LT.excused(t64, bar_z)
    n = side.shape[1]
    for b in range(side.shape[0]):
        nd, nbad = int(diff[b].sum()), int((diff[b] & ~ok[b]).sum())
        print(what, "problem", b, "side differs on", nd, "of", n, "outside the margin:", nbad)
        if nbad or nd > 0.01 * n:
            bad.append(("side", b, nd, nbad))
    return bad


@pytest.mark.parametrize("key", list(LT.ROWS))
def test_row_against_the_truth(dev, cus, monkeypatch, key):
    r = LT.ROWS[key]
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in LT.l1_inputs(r, B)]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    ctl = _control(r)
    before = dict(ctl)
    sol = L.torch_solve_box_qp_l1(*args, ctl)
    st, bad = sol["_stats"], []
    if ctl != before:
        bad.append(("control mutated", {k: (before.get(k), ctl.get(k)) for k in set(ctl) | set(before) if before.get(k) != ctl.get(k)}))
    if r["ctl"].get("sync", True) is False:
        # the module's un-synchronised path: the same schedule, enqueued whole; nothing reports back but the device's status block
        x = L.SolveBoxQPL1(control=_control(r, sync=False))(*args)
        mst = SB.last_forward_status(dev)
        if mst["iters"] != r["K"] or not torch.equal(x, sol["x"]):
            bad.append(("sync=False", mst["iters"], bool(torch.equal(x, sol["x"]))))
    idx, t32, t64 = LT.row_truth(key, cus)
    if sol["iter"] != r["K"]:
        bad.append(("iter", sol["iter"], r["K"]))
    print(key, "stats", {k: st[k] for k in ("linsolve_used", "loop_workgroups", "factor_launches", "mode_used", "loop_kind", "n_factor")})
    bad += [("sig", k, st[k], v) for k, v in r["sig"].items() if st[k] != v]
    if st["n_factor"] != t64["n_factor"] or (t32 is not None and t32["n_factor"] != t64["n_factor"]):
        bad.append(("n_factor", st["n_factor"], t64["n_factor"]))
    res = T.compare(r, {k: _pick(sol[k], idx) for k in VALUES}, t32, t64, keys=VALUES)
    _report(key, res)
    bad += [("value", k, rec) for k, rec in res.items() if not rec["ok"]]
    bad += _side_check(key, _pick(sol["side"], idx), t64, res["z"]["bar"])
    assert not bad, (key, bad)


@pytest.mark.parametrize("name", LT.SAME_BITS)
def test_w_zero_is_the_plain_forward_bit_for_bit(dev, cus, monkeypatch, name):
    r = dict(T.ROW_BY_NAME[name], l1="plain", alpha=1.0)
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in LT.l1_inputs(r, B)]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    plain = L.torch_solve_box_qp(*args[:6], _control(r))
    zero = L.torch_solve_box_qp_l1(*args[:6], torch.zeros_like(args[6]), args[7], _control(r))
    assert plain["iter"] == zero["iter"] == r["K"]
    assert all(zero["_stats"][k] == v for k, v in r["sig"].items() if k != "n_factor"), zero["_stats"]
    assert torch.equal(plain["x"], zero["x"])
    assert torch.equal(plain["z"], zero["z"]) and torch.equal(plain["u"], zero["u"])
    assert float(zero["side"].abs().min()) == 1.0          # (t = 0: no kink set)


@pytest.mark.parametrize("name", list(LT.GRAD_ROWS))
def test_all_eight_gradients_through_the_module(dev, cus, monkeypatch, name):
    r = LT.GRAD_ROWS[name]
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in LT.l1_inputs(r, B)]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in args]
    cot = LT.cot_of(r, B, args[1].dtype)
    x = L.SolveBoxQPL1(control=_control(r))(*leaves)
    mst = SB.last_forward_status(dev)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    assert mst["iters"] == r["K"] and all(mst[{"loop_workgroups": "loop_workgroups_per_qp"}.get(k, k)] == v for k, v in r["sig"].items()
                                          if k != "factor_launches"), mst
    idx, t32, t64 = LT.row_truth(name, cus, "GRAD_ROWS")
    sub = LT.l1_inputs(r, B, idx)
    g64 = LT.truth_grads(r, sub, t64, cot[idx], torch.float64)
    g32 = LT.truth_grads(r, sub, t32, cot[idx], torch.float32) if t32 is not None else None
    order = dict(zip(("dQ", "dp", "dA", "db", "dlb", "dub", "dw", "dc"), leaves))
    res = T.compare(r, {k: _pick(t.grad, idx) for k, t in order.items() if t is not None}, g32, g64, keys=LT.GRADS8)
    res.update(T.compare(r, {"x": _pick(x, idx)}, t32, t64, keys=("x",)))
    _report(name, res)
    bad = [(k, rec) for k, rec in res.items() if not rec["ok"]]
    assert not bad, (name, bad)


def test_a_solve_that_stops_by_itself_takes_the_truths_iterations(dev):
    args = [t.to(dev) for t in LT.stop_inputs(torch.float32)]
    sol = L.torch_solve_box_qp_l1(*args, O.make_control(**LT.STOP_CONTROL))
    t32, t64 = LT.stop_truth(torch.float32), LT.stop_truth(torch.float64)
    print("stop", sol["iter"], t32["iter"], t64["iter"])
    assert sol["iter"] == t64["iter"] == t32["iter"]
    res = T.compare(LT.STOP_ROW, {"x": sol["x"].cpu()}, t32, t64, keys=("x",))
    _report("stop", res)
    assert res["x"]["ok"], res


def test_no_result_depends_on_what_the_new_memory_held(dev, cus, monkeypatch):
    """In the manner of tests/mem_table.py, on tests/memharness.py: every workspace (the new regions ws, cs, t behind the forward's
    layout among them), output and temporary of a forward and a backward through the module is a guarded buffer filled with 0x00,
    then with 0xFF -- the same bits come back, no guard is touched."""
    import memharness as H
    r = LT.ROWS["wide_n1025_f32-K10"]          # (n > 1024: the one shape class at which the t third of the L1 area is read)
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in LT.l1_inputs(r, B)]
    lib = _lib.load()
    dt = _lib.dtype_code(args[1])
    assert lib.lqp_boxqp_forward_l1_workspace_bytes(dt, B, r["n"], r["m"]) > lib.lqp_boxqp_forward_workspace_bytes(dt, B, r["n"], r["m"])
    outs = []
    for fill in (0x00, 0xFF):
        H.release(_lib)
        with H.controlled_memory(monkeypatch, fill):
            sol = L.torch_solve_box_qp_l1(*args, _control(r))
            leaves = [None if t is None else t.clone().requires_grad_(True) for t in args]
            x = L.SolveBoxQPL1(control=_control(r))(*leaves)
            x.backward(LT.cot_of(r, B, x.dtype).to(dev))
            torch.cuda.synchronize()
            got = {k: sol[k].clone() for k in ("x", "z", "u", "lams", "side", "u_box")}          # (m = 0 at this shape: no nus)
            got.update({"x_module": x.detach().clone()}, **{"d" + str(k): t.grad.clone() for k, t in enumerate(leaves) if t is not None})
            assert sol["iter"] == r["K"]
        assert H.check_guards() == [] and H.check_inputs_untouched() == []
        outs.append(got)
    H.release(_lib)
    assert len(outs[0]) == 6 + 1 + sum(t is not None for t in args)
    for k in outs[0]:
        assert H.same_bits(outs[0][k], outs[1][k]), k
    assert bool(torch.isfinite(outs[1]["side"]).all()) and bool(torch.isfinite(outs[1]["u_box"]).all())


def test_a_negative_or_non_finite_weight_is_refused_on_the_device(dev):
    """checked where the data are: the call that waits raises the package's ValueError and names the problem"""
    r = LT.ROWS["small_n31_m1-K10"]
    args = [None if t is None else t.to(dev) for t in LT.l1_inputs(r, 4)]
    for bad in (-1e-3, float("nan"), float("inf")):
        w = args[6].clone()
        w[2, 5, 0] = bad
        with pytest.raises(ValueError, match=r"w must be finite and >= 0, and rho positive and finite \(batch index 2\)"):
            L.torch_solve_box_qp_l1(*args[:6], w, args[7], _control(r))
    # ... and a per-problem rho: t = ws / rho is a threshold only for a positive one
    for bad in (0.0, -1.0):
        rho = torch.ones(4, 1, 1, device=dev)
        rho[1] = bad
        with pytest.raises(ValueError, match=r"rho positive and finite \(batch index 1\)"):
            L.torch_solve_box_qp_l1(*args, _control(r, rho=rho))
    sol = L.torch_solve_box_qp_l1(*args, _control(r))          # (the workspace and the layer are as good as before)
    assert sol["iter"] == r["K"] and bool(torch.isfinite(sol["x"]).all())
