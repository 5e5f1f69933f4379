"""The soft-band layer on the GPU: every row of tests/soft_table.py against its truth at a pinned iteration count, zero weights
against the plain forward and lo = hi, wl = wu against the L1 layer bit for bit, all ten gradients through the module, a solve that
stops by itself, a memory row, the refusals made on the device, sync=False.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale, t32 / t64 the
truth (soft_table.solve_soft) in float32 / float64.  `zone` is compared exactly; an element may differ only where the float64 truth
says it sits within the bar for z of changing its set (soft_table.excused), and at most 1 % of a problem's elements may.
tests/test_soft_table.py shows, without a GPU, that the iterates of the plain step and of the L1 step around the band's middle miss
every row's bar for z by at least 100 x.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import soft_table as ST
import tier_table as T

pytestmark = pytest.mark.gpu
HIP_KEYS = ("linsolve", "launch_mode")
VALUES = tuple(k for k in ST.OUTPUTS if k != "zone")
# (the gradients' bars are the ones tests/test_gpu_fp.py uses, fp_table.compare: tier_table.compare over every gradient; the four new
#  ones take them like dp and dlb)


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


def _zone_check(what, zone, t64, bar_z):
    """-> list of failures: `zone` against the float64 truth's, exact outside the margin, at most 1 % of a problem inside it"""
    bad = []
    diff = zone.double() != t64["zone"]
    ok = ST.excused(t64, bar_z)
    n = zone.shape[1]
    for b in range(zone.shape[0]):
        nd, nbad = int(diff[b].sum()), int((diff[b] & ~ok[b]).sum())
        print(what, "problem", b, "zone differs on", nd, "of", n, "outside the margin:", nbad)
        if nbad or nd > 0.01 * n:
            bad.append(("zone", b, nd, nbad))
    return bad


@pytest.mark.parametrize("key", list(ST.ROWS))
def test_row_against_the_truth(dev, cus, monkeypatch, key):
    r = ST.ROWS[key]
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, B)]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    ctl = _control(r)
    before = dict(ctl)
    sol = L.torch_solve_box_qp_soft(*args, ctl)
    st, bad = sol["_stats"], []
    if ctl != before:
        bad.append(("control mutated", {k: (before.get(k), ctl.get(k)) for k in set(ctl) | set(before) if before.get(k) != ctl.get(k)}))
    if r["ctl"].get("sync", True) is False:
        # the module's un-synchronised path: the same schedule, enqueued whole; nothing reports back but the device's status block
        x = L.SolveBoxQPSoft(control=_control(r, sync=False))(*args)
        mst = SB.last_forward_status(dev)
        L.synchronize()
        if mst["iters"] != r["K"] or not torch.equal(x, sol["x"]):
            bad.append(("sync=False", mst["iters"], bool(torch.equal(x, sol["x"]))))
    idx, t32, t64 = ST.row_truth(key, cus)
    if sol["iter"] != r["K"]:
        bad.append(("iter", sol["iter"], r["K"]))
    print(key, "stats", {k: st[k] for k in ("linsolve_used", "loop_workgroups", "factor_launches", "mode_used", "loop_kind", "n_factor")})
    bad += [("sig", k, st[k], v) for k, v in r["sig"].items() if st[k] != v]
    if st["n_factor"] != t64["n_factor"] or (t32 is not None and t32["n_factor"] != t64["n_factor"]):
        bad.append(("n_factor", st["n_factor"], t64["n_factor"]))
    res = T.compare(r, {k: _pick(sol[k], idx) for k in VALUES}, t32, t64, keys=VALUES)
    _report(key, res)
    bad += [("value", k, rec) for k, rec in res.items() if not rec["ok"]]
    bad += _zone_check(key, _pick(sol["zone"], idx), t64, res["z"]["bar"])
    assert not bad, (key, bad)


@pytest.mark.parametrize("name", ST.SAME_BITS)
def test_zero_weights_are_the_plain_forward_bit_for_bit(dev, cus, monkeypatch, name):
    r = dict(T.ROW_BY_NAME[name], soft="plain", l1="plain", alpha=1.0)
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, B)]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    plain = L.torch_solve_box_qp(*args[:6], _control(r))
    zero = L.torch_solve_box_qp_soft(*args[:6], torch.zeros_like(args[6]), torch.zeros_like(args[7]), args[8], args[9], _control(r))
    assert plain["iter"] == zero["iter"] == r["K"]
    assert all(zero["_stats"][k] == v for k, v in r["sig"].items() if k != "n_factor"), zero["_stats"]
    assert torch.equal(plain["x"], zero["x"])
    assert torch.equal(plain["z"], zero["z"]) and torch.equal(plain["u"], zero["u"])
    assert not bool((zero["zone"].abs() == 1).any())          # (no weight, no kink set)


@pytest.mark.parametrize("name", ST.L1EQ_ROWS)
def test_l1eq_is_the_l1_layer_bit_for_bit(dev, cus, monkeypatch, name):
    """lo = hi = c, wl = wu = w on the same device: the L1 kernels, pinned by tests/test_gpu_l1.py, are the reference"""
    r = dict(T.ROW_BY_NAME[name], soft="l1eq", l1="plain", alpha=ST.LT.ALPHA if name in ST.LT.RELAXED else 1.0)
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, B)]
    assert torch.equal(args[6], args[7]) and torch.equal(args[8], args[9])
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    l1 = L.torch_solve_box_qp_l1(*args[:6], args[6], args[8], _control(r))
    soft = L.torch_solve_box_qp_soft(*args, _control(r))
    assert l1["iter"] == soft["iter"] == r["K"]
    for k in ("loop_kind", "loop_workgroups", "linsolve_used", "mode_used", "n_factor"):
        assert l1["_stats"][k] == soft["_stats"][k], (k, l1["_stats"], soft["_stats"])
    for k in ("x", "z", "u", "u_box", "lams"):
        assert torch.equal(l1[k], soft[k]), k
    zone, side = soft["zone"], l1["side"]
    assert torch.equal(zone.abs() == 1, side == 0) and int((side == 0).sum()) > 0
    assert torch.equal(torch.where(zone.abs() == 2, zone / 2, torch.zeros_like(zone)), side)


@pytest.mark.parametrize("name", list(ST.GRAD_ROWS))
def test_all_ten_gradients_through_the_module(dev, cus, monkeypatch, name):
    r = ST.GRAD_ROWS[name]
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, B)]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in args]
    cot = ST.cot_of(r, B, args[1].dtype)
    x = L.SolveBoxQPSoft(control=_control(r))(*leaves)
    mst = SB.last_forward_status(dev)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    assert mst["iters"] == r["K"] and all(mst[{"loop_workgroups": "loop_workgroups_per_qp"}.get(k, k)] == v for k, v in r["sig"].items()
                                          if k != "factor_launches"), mst
    idx, t32, t64 = ST.row_truth(name, cus, "GRAD_ROWS")
    sub = ST.soft_inputs(r, B, idx)
    g64 = ST.truth_grads(r, sub, t64, cot[idx], torch.float64)
    g32 = ST.truth_grads(r, sub, t32, cot[idx], torch.float32) if t32 is not None else None
    order = dict(zip(ST.GRADS10, leaves))
    assert all(t.grad is not None for t in order.values() if t is not None)
    res = T.compare(r, {k: _pick(t.grad, idx) for k, t in order.items() if t is not None}, g32, g64, keys=ST.GRADS10)
    res.update(T.compare(r, {"x": _pick(x, idx)}, t32, t64, keys=("x",)))
    _report(name, res)
    assert set(res) == set(ST.GRADS10) | {"x"}
    for k in ("dwl", "dwu", "dlo", "dhi"):
        assert float(g64[k].abs().max()) > 0, k          # (the new gradients are not trivially zero)
    bad = [(k, rec) for k, rec in res.items() if not rec["ok"]]
    assert not bad, (name, bad)


def test_a_solve_that_stops_by_itself_takes_the_truths_iterations(dev):
    args = [t.to(dev) for t in ST.stop_inputs(torch.float32)]
    sol = L.torch_solve_box_qp_soft(*args, O.make_control(**ST.STOP_CONTROL))
    t32, t64 = ST.stop_truth(torch.float32), ST.stop_truth(torch.float64)
    print("stop", sol["iter"], t32["iter"], t64["iter"])
    assert sol["iter"] == t64["iter"] == t32["iter"]
    res = T.compare(ST.STOP_ROW, {"x": sol["x"].cpu()}, t32, t64, keys=("x",))
    _report("stop", res)
    assert res["x"]["ok"], res


def test_no_result_depends_on_what_the_new_memory_held(dev, cus, monkeypatch):
    """In the manner of tests/mem_table.py, on tests/memharness.py: every workspace (the six new regions behind the forward's layout
    among them), output and temporary of a forward and a backward through the module is a guarded buffer filled with 0x00, then with
    0xFF -- the same bits come back, no guard is touched."""
    import memharness as H
    r = ST.ROWS["wide_n1025_f32-K10"]          # (n > 1024: the one shape class at which the tl / tu regions are read)
    B = T.batch(r, cus)
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, B)]
    lib = _lib.load()
    dt = _lib.dtype_code(args[1])
    assert lib.lqp_boxqp_forward_soft_workspace_bytes(dt, B, r["n"], r["m"]) > lib.lqp_boxqp_forward_l1_workspace_bytes(dt, B, r["n"], r["m"])
    outs = []
    for fill in (0x00, 0xFF):
        H.release(_lib)
        with H.controlled_memory(monkeypatch, fill):
            sol = L.torch_solve_box_qp_soft(*args, _control(r))
            leaves = [None if t is None else t.clone().requires_grad_(True) for t in args]
            x = L.SolveBoxQPSoft(control=_control(r))(*leaves)
            x.backward(ST.cot_of(r, B, x.dtype).to(dev))
            torch.cuda.synchronize()
            got = {k: sol[k].clone() for k in ("x", "z", "u", "lams", "zone", "u_box")}          # (m = 0 at this shape: no nus)
            got.update({"x_module": x.detach().clone()}, **{"d" + str(k): t.grad.clone() for k, t in enumerate(leaves) if t is not None})
            assert sol["iter"] == r["K"]
        assert H.check_guards() == [] and H.check_inputs_untouched() == []
        outs.append(got)
    H.release(_lib)
    assert len(outs[0]) == 6 + 1 + sum(t is not None for t in args)
    for k in outs[0]:
        assert H.same_bits(outs[0][k], outs[1][k]), k
    assert bool(torch.isfinite(outs[1]["zone"]).all()) and bool(torch.isfinite(outs[1]["u_box"]).all())


MESSAGE = r"wl and wu must be finite and >= 0, lo <= hi without NaN, and rho positive and finite \(batch index %d\)"


def test_bad_band_data_are_refused_on_the_device(dev):
    """checked where the data are: the call that waits raises the package's ValueError and names the problem; the next call works"""
    r = ST.ROWS["small_n31_m1-K10"]
    args = [None if t is None else t.to(dev) for t in ST.soft_inputs(r, 4)]

    def solve(**over):
        a = list(args)
        for k, v in over.items():
            a[dict(wl=6, wu=7, lo=8, hi=9)[k]] = v
        return L.torch_solve_box_qp_soft(*a, _control(r))

    def planted(k, b, value):
        t = args[dict(wl=6, wu=7, lo=8, hi=9)[k]].clone()
        t[b, 5, 0] = value
        return {k: t}
    # a bad weight, on either side
    for k in ("wl", "wu"):
        for value in (-1e-3, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=MESSAGE % 2):
                solve(**planted(k, 2, value))
    # lo > hi
    with pytest.raises(ValueError, match=MESSAGE % 3):
        solve(**planted("lo", 3, float(args[9][3, 5, 0]) + 0.25))
    with pytest.raises(ValueError, match=MESSAGE % 0):
        solve(**planted("lo", 0, float("inf")))
    # NaN in lo or hi
    for k in ("lo", "hi"):
        with pytest.raises(ValueError, match=MESSAGE % 1):
            solve(**planted(k, 1, float("nan")))
    # an infinite kink on its own side is data, not an error
    ok = solve(**planted("lo", 1, -float("inf")), **planted("hi", 2, float("inf")))
    assert ok["iter"] == r["K"] and bool(torch.isfinite(ok["x"]).all())
    # a per-problem rho: tl, tu are thresholds only for a positive, finite one
    for value in (0.0, -1.0, float("inf")):
        rho = torch.ones(4, 1, 1, device=dev)
        rho[1] = value
        with pytest.raises(ValueError, match=MESSAGE % 1):
            L.torch_solve_box_qp_soft(*args, _control(r, rho=rho))
    sol = solve()          # (the workspace and the layer are as good as before)
    assert sol["iter"] == r["K"] and bool(torch.isfinite(sol["x"]).all())
