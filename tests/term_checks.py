"""The bodies the tests of the separable-term layers share, each written once as a function of the term's record (``term_table.Table``)
and, on the GPU, of the layer: (record, forward entry point, module class).  tests/test_{l1,soft,log,pwl}_table.py call the CPU half,
tests/test_gpu_{l1,soft,log,pwl}.py the GPU half and import the fixtures `dev` and `cus` by name.  What differs for one term stays in
that term's module: a body here returns what it computed, and the module goes on from there.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale.  The record's
label (`side`, `zone`, the clamped set, `piece`) is compared exactly; an element may differ only where the float64 truth says it sits
within the bar for z of changing its set (term_table.excused), and at most 1 % of a problem's elements may.
"""
import pytest
import torch

from oracle import boxqp_oracle as O
import l1_table as LT
import term_table as TT
import tier_table as T

CUS = 256          # the compute units of an MI355X: the batch sizes the GPU test will see
HIP_KEYS = ("linsolve", "launch_mode")


@pytest.fixture(scope="module")
def dev():
    from lqp_py_amd import _lib
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


def _on_dev(inp, dev):
    return [None if t is None else t.to(dev) for t in inp]


def _row_on_dev(rec, r, dev, cus, monkeypatch):
    """-> (B, the row's inputs on the device), the row's environment set"""
    B = T.batch(r, cus)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    return B, _on_dev(rec.inputs(r, B), dev)


def _set_check(rec, what, got, t64, bar_z):
    """-> list of failures: the record's label of `got` against the float64 truth's, exact outside the margin, at most 1 % of a
    problem inside it"""
    bad = []
    diff = rec.label(got) != rec.label(t64)
    ok = TT.excused(t64, bar_z)
    n = diff.shape[1]
    for b in range(diff.shape[0]):
        nd, nbad = int(diff[b].sum()), int((diff[b] & ~ok[b]).sum())
        print(what, "problem", b, rec.what, "differs on", nd, "of", n, "outside the margin:", nbad)
        if nbad or nd > 0.01 * n:
            bad.append((rec.what, b, nd, nbad))
    return bad


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def row_against_the_truth(layer, dev, cus, monkeypatch, key):
    """-> (args, picked outputs, idx, t32, t64, res) of a row that met its bars"""
    import lqp_py_amd as L
    import lqp_py_amd.solve_box_qp_admm_torch as SB
    rec, entry, module = layer
    r = rec.tables["ROWS"][key]
    B, args = _row_on_dev(rec, r, dev, cus, monkeypatch)
    ctl = _control(r)
    before = dict(ctl)
    sol = entry(*args, ctl)
    st, bad = sol["_stats"], []
    if ctl != before:
        bad.append(("control mutated", {k: (before.get(k), ctl.get(k)) for k in set(ctl) | set(before) if before.get(k) != ctl.get(k)}))
    if r["ctl"].get("sync", True) is False:
        # the module's un-synchronised path: the same schedule, enqueued whole; nothing reports back but the device's status block
        x = module(control=_control(r, sync=False))(*args)
        mst = SB.last_forward_status(dev)
        L.synchronize()
        if mst["iters"] != r["K"] or not torch.equal(x, sol["x"]):
            bad.append(("sync=False", mst["iters"], bool(torch.equal(x, sol["x"]))))
    idx, t32, t64 = rec.row_truth(key, cus)
    if sol["iter"] != r["K"]:
        bad.append(("iter", sol["iter"], r["K"]))
    print(key, "stats", {k: st[k] for k in ("linsolve_used", "loop_workgroups", "factor_launches", "mode_used", "loop_kind", "n_factor")})
    bad += [("sig", k, st[k], v) for k, v in r["sig"].items() if st[k] != v]
    if st["n_factor"] != t64["n_factor"] or (t32 is not None and t32["n_factor"] != t64["n_factor"]):
        bad.append(("n_factor", st["n_factor"], t64["n_factor"]))
    got = {k: _pick(sol[k], idx) for k in T.OUTPUTS + (rec.aux, "u_box")}
    values = tuple(k for k in got if k != rec.aux)
    res = T.compare(r, got, t32, t64, keys=values)
    _report(key, res)
    bad += [("value", k, v) for k, v in res.items() if not v["ok"]]
    bad += _set_check(rec, key, got, t64, res["z"]["bar"])
    assert not bad, (key, bad)
    return args, got, idx, t32, t64, res


def zero_term_is_the_plain_forward(layer, dev, cus, monkeypatch, name):
    """-> the solution of the layer at zero weights: the plain forward's x, z, u bit for bit, at the row's signature"""
    import lqp_py_amd as L
    rec, entry, _ = layer
    r = dict(T.ROW_BY_NAME[name], alpha=1.0)          # (no kind: every table's data generator takes that for "plain")
    B, args = _row_on_dev(rec, r, dev, cus, monkeypatch)
    plain = L.torch_solve_box_qp(*args[:6], _control(r))
    zero = entry(*args[:6], *[torch.zeros_like(t) for t in args[6:6 + rec.weights]], *args[6 + rec.weights:], _control(r))
    assert plain["iter"] == zero["iter"] == r["K"]
    assert all(zero["_stats"][k] == v for k, v in r["sig"].items() if k != "n_factor"), zero["_stats"]
    assert torch.equal(plain["x"], zero["x"])
    assert torch.equal(plain["z"], zero["z"]) and torch.equal(plain["u"], zero["u"])
    return zero


def gradients_through_the_module(layer, dev, cus, monkeypatch, name):
    """-> (res, the device's gradients picked, g64, t64, sub, cot of the sampled problems) of a gradient row that met its bars"""
    import lqp_py_amd.solve_box_qp_admm_torch as SB
    rec, _, module = layer
    r = rec.tables["GRAD_ROWS"][name]
    B, args = _row_on_dev(rec, r, dev, cus, monkeypatch)
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in args]
    cot = TT.cot_of(r, B, args[1].dtype)
    x = module(control=_control(r))(*leaves)
    mst = SB.last_forward_status(dev)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    assert mst["iters"] == r["K"] and all(mst[{"loop_workgroups": "loop_workgroups_per_qp"}.get(k, k)] == v for k, v in r["sig"].items()
                                          if k != "factor_launches"), mst
    idx, t32, t64 = rec.row_truth(name, cus, "GRAD_ROWS")
    sub = rec.inputs(r, B, idx)
    g64 = rec.truth_grads(r, sub, t64, cot[idx], torch.float64)
    g32 = rec.truth_grads(r, sub, t32, cot[idx], torch.float32) if t32 is not None else None
    order = dict(zip(rec.grads, leaves))
    assert all(t.grad is not None and t.grad.shape == t.shape for t in order.values() if t is not None)
    hip = {k: _pick(t.grad, idx) for k, t in order.items() if t is not None}
    # (the bars are the ones tests/test_gpu_fp.py uses, fp_table.compare: tier_table.compare over every gradient; the term's own
    #  gradients take them like dp and dlb)
    res = T.compare(r, hip, g32, g64, keys=rec.grads)
    res.update(T.compare(r, {"x": _pick(x, idx)}, t32, t64, keys=("x",)))
    _report(name, res)
    assert set(res) == set(rec.grads) | {"x"}
    bad = [(k, v) for k, v in res.items() if not v["ok"]]
    assert not bad, (name, bad)
    return res, hip, g64, t64, sub, cot[idx]


def stopped_solve_takes_the_truths_iterations(layer, dev):
    rec, entry, _ = layer
    args = [t.to(dev) for t in rec.stop_inputs(torch.float32)]
    sol = entry(*args, O.make_control(**TT.STOP_CONTROL))
    t32, t64 = rec.stop_truth(torch.float32), rec.stop_truth(torch.float64)
    print("stop", sol["iter"], t32["iter"], t64["iter"])
    assert sol["iter"] == t64["iter"] == t32["iter"]
    res = T.compare(TT.STOP_ROW, {"x": sol["x"].cpu()}, t32, t64, keys=("x",))
    _report("stop", res)
    assert res["x"]["ok"], res


def no_result_depends_on_what_the_new_memory_held(layer, dev, cus, monkeypatch, smaller):
    """The row above 1024 elements (the one shape class at which the term's regions of the workspace are read) in the manner of
    tests/mem_table.py, on tests/memharness.py.  `smaller`: the name of a workspace query this layer's must exceed."""
    import memharness as H
    from lqp_py_amd import _lib
    rec, entry, module = layer
    r = rec.tables["ROWS"]["wide_n1025_f32-K10"]
    B = T.batch(r, cus)
    args = _on_dev(rec.inputs(r, B), dev)
    lib = _lib.load()
    size = (_lib.dtype_code(args[1]), B, r["n"], r["m"])
    assert getattr(lib, "lqp_boxqp_forward_%s_workspace_bytes" % rec.name)(*size) > getattr(lib, smaller)(*size)
    keys = ("x", "z", "u", "lams", rec.aux, "u_box")          # (m = 0 at this shape: no nus)
    outs = []
    for fill in (0x00, 0xFF):
        H.release(_lib)
        with H.controlled_memory(monkeypatch, fill):
            sol = entry(*args, _control(r))
            leaves = [None if t is None else t.clone().requires_grad_(True) for t in args]
            x = module(control=_control(r))(*leaves)
            x.backward(TT.cot_of(r, B, x.dtype).to(dev))
            torch.cuda.synchronize()
            got = {k: sol[k].clone() for k in keys}
            got.update({"x_module": x.detach().clone()}, **{"d" + str(k): t.grad.clone() for k, t in enumerate(leaves) if t is not None})
            assert sol["iter"] == r["K"]
        assert H.check_guards() == [] and H.check_inputs_untouched() == []
        outs.append(got)
    H.release(_lib)
    assert len(outs[0]) == 6 + 1 + sum(t is not None for t in args)
    for k in outs[0]:
        assert H.same_bits(outs[0][k], outs[1][k]), k
    assert bool(torch.isfinite(outs[1][rec.aux]).all()) and bool(torch.isfinite(outs[1]["u_box"]).all())


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def row_needs_the_step(rec, key):
    """A row is pinned to its K, the iterates of the other steps are at least 100 bars away (a kernel without the step cannot pass),
    the label of the float32 truth is the float64 truth's -- exact outside the margin, under the 1 % cap inside it --, and the event
    row's event fires.  -> (r, idx, t32, t64, the sampled problems' inputs)"""
    r = rec.tables["ROWS"][key]
    idx, t32, t64 = rec.row_truth(key, CUS)
    n = r["n"]
    assert t64["iter"] == r["K"]
    sub = rec.inputs(r, T.batch(r, CUS), idx)
    dt = torch.float32 if r["dtype"] == "f32" else torch.float64
    for step in rec.steps_of(r[rec.name]):
        other = rec.truth(r, sub, dt, step=step)
        res = T.compare(r, {k: other[k] for k in rec.far_keys}, t32, t64, keys=rec.far_keys)
        for k, v in res.items():
            assert v["err"] >= 100 * v["bar"], (key, step, k, v)
    if t32 is not None:
        zbar = T.compare(r, {"z": t32["z"]}, t32, t64, keys=("z",))["z"]["bar"]
        diff = rec.label(t32) != rec.label(t64)
        assert not bool((diff & ~TT.excused(t64, zbar)).any()), key
        assert all(int(d.sum()) <= 0.01 * n for d in diff), key
        assert t32["n_factor"] == t64["n_factor"]
    if key.startswith(LT.EVENT_ROW):
        assert t64["n_factor"] == 2           # (the event at iteration 100 fires: the thresholds change with rho)
    return r, idx, t32, t64, sub


def row_holds_its_sets(rec, key, r, s, problems):
    """Every set of `s` (name -> bool (B, n, 1)) holds the record's share of every sampled problem -- below `pooled_below` elements of
    the row's sampled problems together: a single small problem can have an empty set --, but the sets the kind empties by construction"""
    n, empty = r["n"], rec.empty.get(r[rec.name], ())
    for k, v in s.items():
        sizes = [int(q.sum()) for q in v]
        if k in empty:
            assert sum(sizes) == 0, (key, k)
        elif n >= rec.pooled_below:
            assert all(q >= rec.share * n for q in sizes), (key, k, sizes)
        else:
            assert sum(sizes) >= rec.share * n * problems, (key, k, sum(sizes))


def gradient_row_in_both_precisions(rec, name):
    """The label and the clamped set of a gradient row are the same in float32 and float64.  -> (r, idx, t32, t64, inputs)"""
    r = rec.tables["GRAD_ROWS"][name]
    idx, t32, t64 = rec.row_truth(name, CUS, "GRAD_ROWS")
    sub = rec.inputs(r, T.batch(r, CUS), idx)
    if t32 is None:
        t32 = rec.truth(r, sub, torch.float32)
    assert torch.equal(rec.label(t32), rec.label(t64)), name
    assert torch.equal(t32["u_box"] != 0, t64["u_box"] != 0), name
    return r, idx, t32, t64, sub


def stopped_solve_stops_at_one_count(rec):
    t32, t64 = rec.stop_truth(torch.float32), rec.stop_truth(torch.float64)
    assert t32["iter"] == t64["iter"] and 0 < t64["iter"] < 9999
    plain = O.solve_box_qp(*rec.stop_inputs(torch.float64)[:6], O.make_control(**TT.STOP_CONTROL))
    assert float((plain["x"] - t64["x"]).abs().max()) > 1e-2


def central_differences(rec, args, cot, ctl, sol, leave_out=None):
    """d(cot' x*) / d(every entry of every argument) by central differences of the truth against the record's gradient recipe at
    `sol`.  leave_out: {gradient name: bool tensor} -- entries at which only a one-sided derivative exists.  -> the recipe's gradients"""
    got = rec.grad_recipe(cot, sol, args[0], args[2], args[4], args[5], *[args[6 + k] for k in rec.recipe_data])
    h = 1e-6
    for k, name in enumerate(rec.grads):
        t = args[k]
        fd = torch.zeros_like(t)
        flat, out = t.reshape(-1), fd.reshape(-1)
        skip = None if leave_out is None or name not in leave_out else leave_out[name].reshape(-1)
        for e in range(flat.numel()):
            if skip is not None and bool(skip[e]):
                continue
            vals = []
            for sgn in (1, -1):
                tt = flat.clone()
                tt[e] += sgn * h
                a2 = list(args)
                a2[k] = tt.reshape(t.shape)
                if k == 0:      # (dQ is the gradient with respect to a symmetric perturbation: the reference's (dv x' + x dv') / 2)
                    a2[0] = 0.5 * (a2[0] + a2[0].transpose(1, 2))
                vals.append(float((cot * rec.solve(*a2, ctl)["x"]).sum()))
            out[e] = (vals[0] - vals[1]) / (2 * h)
        ref = got[name]
        err = float((fd - ref).abs().max())
        print(name, "max |fd - recipe| %.2e" % err, "scale %.2e" % float(ref.abs().max()))
        assert err < 2e-5 * max(1.0, float(ref.abs().max())), (name, err)
    return got
