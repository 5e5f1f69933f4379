"""Every row of tests/direct_table.py on the GPU: the entry points that do not run the ADMM loop, against the CPU oracle.  GPU only.

One test per family over its rows.  The truth is the oracle in float64 on the row's (rounded) inputs, the budget the same function
in float32: float32 rows |hip - t64| <= R |t32 - t64| + F scale, float64 rows |hip - t64| <= 1e-9 scale (tier_table.compare).
Beside the numbers: a solve returns the caller's shape and dtype and leaves the caller's tensor alone, a second solve with the
same packed factor and a solve with a freshly packed one give the same bits; `same` rows give the bits of the run without their
environment override; the no-bound layer reports iter == 0, no finite bound, the LU x-update, u == 0 and lams == 0 exactly, and
writes rho = 0 into the caller's control.  Every ratio goes to the session's parity report, case "direct:<row>".
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib, lu_layer
import lqp_py_amd.solve_box_qp_admm_torch as SB
import direct_table as DT
import parity_report as P

pytestmark = pytest.mark.gpu
GRADS6 = ("dQ", "dp", "dA", "db", "dlb", "dub")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _names(family, singular=False):
    return [r["name"] for r in DT.rows_of(family, singular)]


def _gpu(inp, dev, *keys):
    return [None if inp[k] is None else inp[k].to(dev) for k in keys]


def _cpu(d):
    return {k: (None if v is None else v.detach().cpu()) for k, v in d.items()}


def _truths(r, inp):
    return DT.truth(r, inp, torch.float64), (DT.truth(r, inp, torch.float32) if r["dtype"] == "f32" else None)


def _judge(r, hip, t32, t64, bad, tag=""):
    """Compare, print, record under case "direct:<row>" (outputs named tag + key); failures go to `bad`."""
    case = f"direct:{r['name']}"
    res = DT.compare(r, _cpu(hip), t32, t64, keys=tuple(k for k in t64 if k in hip))
    missing = sorted(k for k in hip if k in t64 and k not in res)
    if missing:
        bad.append(("not returned", tag, missing))
    for k, rec in res.items():
        print(f"{case} {tag}{k}: err {rec['err']:.3e} budget {rec.get('budget', float('nan')):.3e} ratio {rec.get('ratio', float('nan')):.3g} "
              f"bar {rec['bar']:.3e} scale {rec['scale']:.3g} ok {rec['ok']}")
        P.record(case, tag + k, rec["err"], rec["scale"], ratio=rec.get("ratio"), budget=rec.get("budget"), bar=rec["bar"],
                 R=r["R"], F=r["F"], dtype=r["dtype"])
        if not rec["ok"]:
            bad.append(("value", tag + k, rec))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# lu_factor / lu_solve / _PackedFactor.solve
def _solve_once(r, inp, dev):
    """Factor (the row's source), a one-off lu_solve, two solves with one packed factor -> (three results, the rhs given, its copy)."""
    M = inp["M"]
    if r["factor"] == "torch":
        LU, piv = (t.to(dev) for t in torch.linalg.lu_factor(M))
    else:
        LU, piv = lu_layer.lu_factor(M.to(dev))
    rhs = DT.shape_rhs(r, inp["base"].to(dev))
    before = rhs.clone()
    xa = lu_layer.lu_solve(LU, piv, rhs)
    pf = lu_layer._PackedFactor(LU, piv)
    x1, x2 = pf.solve(rhs), pf.solve(rhs)
    torch.cuda.synchronize()
    return (xa, x1, x2), rhs, before


@pytest.mark.parametrize("name", _names("solve"))
def test_solve_against_the_oracle(dev, monkeypatch, name):
    r = DT.ROW_BY_NAME[name]
    inp = DT.inputs(r)
    t64, t32 = _truths(r, inp)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    (xa, x1, x2), rhs, before = _solve_once(r, inp, dev)
    bad = []
    if r["rhs"] == "k3t" and rhs.is_contiguous():
        bad.append(("the transposed right-hand side arrived contiguous",))
    if not (torch.equal(rhs, before) and rhs.stride() == before.stride()):
        bad.append(("the caller's right-hand side changed",))
    for what, x in (("one-off", xa), ("packed", x1), ("packed again", x2)):
        if x.shape != rhs.shape or x.dtype != DT.dtype_of(r) or not x.is_contiguous():
            bad.append(("shape / dtype", what, tuple(x.shape), x.dtype))
    if not torch.equal(x1, x2):
        bad.append(("a second solve with the same packed factor changed bits",))
    if not torch.equal(xa, x1):
        bad.append(("a freshly packed factor changed bits",))
    _judge(r, dict(x=x1), t32, t64, bad)
    if r["same"]:
        for k in r["env"]:
            monkeypatch.delenv(k)
        (ya, y1, _), _, _ = _solve_once(r, inp, dev)
        same = torch.equal(y1, x1) and torch.equal(ya, xa)
        P.record(f"direct:{name}", "flip", 0.0, 1.0, same=same, env=r["env"])
        print(f"direct:{name} without {r['env']}: same bits {same}")
        if not same:
            bad.append(("the override changed bits", r["env"]))
    assert not bad, (name, bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# TorchLU / TorchLULayer
@pytest.mark.parametrize("name", _names("lulayer"))
def test_lu_layer_against_the_oracle(dev, name):
    r = DT.ROW_BY_NAME[name]
    inp = DT.inputs(r)
    t64, t32 = _truths(r, inp)
    M, = _gpu(inp, dev, "M")
    rhs, g = (DT.shape_rhs(r, inp[k].to(dev)) for k in ("base", "gbase"))
    bad = []
    outs = {}
    for tag in ("cached", "uncached"):
        Mg, rg = M.clone().requires_grad_(True), rhs.clone().requires_grad_(True)
        x = L.TorchLU(A=M)(Mg, rg) if tag == "cached" else L.TorchLULayer.apply(Mg, rg)
        x.backward(g)
        torch.cuda.synchronize()
        if x.shape != rhs.shape or rg.grad.shape != rhs.shape or Mg.grad.shape != M.shape:
            bad.append(("shape", tag, tuple(x.shape), tuple(rg.grad.shape), tuple(Mg.grad.shape)))
        outs[tag] = dict(x=x.detach(), dA=Mg.grad, db=rg.grad)
        _judge(r, outs[tag], t32, t64, bad, tag=tag + ".")
    if not all(torch.equal(outs["cached"][k], outs["uncached"][k]) for k in ("x", "dA", "db")):
        bad.append(("the cached factor changed bits",))
    assert not bad, (name, bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# torch_solve_qp_eqcon(_grad), torch_solve_qp_uncon(_grad)
@pytest.mark.parametrize("name", _names("eqcon") + _names("uncon"))
def test_qp_solve_and_grad_against_the_oracle(dev, name):
    r = DT.ROW_BY_NAME[name]
    inp = DT.inputs(r)
    t64, t32 = _truths(r, inp)
    Q, p, A, b, cot = _gpu(inp, dev, "Q", "p", "A", "b", "cot")
    pt = {k: (None if v is None else v.to(dev)) for k, v in DT.point(r, inp).items()}
    if r["family"] == "eqcon":
        sol = L.torch_solve_qp_eqcon(Q, p, A, b)
        g = L.torch_solve_qp_eqcon_grad(cot, pt["x"], pt["nus"], Q, A)
        hip = dict(x=sol["x"], nus=sol["nus"], **dict(zip(GRADS6[:4], g)))
    else:
        sol = L.torch_solve_qp_uncon(Q, p)
        g = L.torch_solve_qp_uncon_grad(cot, pt["x"], Q)
        hip = dict(x=sol["x"], **dict(zip(GRADS6[:2], g)))
    torch.cuda.synchronize()
    bad = []
    if set(hip) != set(t64):
        bad.append(("outputs", sorted(hip), sorted(t64)))
    for k, v in hip.items():
        if v.shape != t64[k].shape or v.dtype != DT.dtype_of(r):
            bad.append(("shape / dtype", k, tuple(v.shape), v.dtype))
    _judge(r, hip, t32, t64, bad)
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", _names("eqcon", singular=True))
def test_singular_kkt_matrix_raises(dev, name):
    """A zero row of A in one problem: an exactly zero pivot whatever the rounding -- an error return, named by its batch element."""
    r = DT.ROW_BY_NAME[name]
    inp = DT.inputs(r)
    assert not bool(inp["A"][r["singular"][0], r["singular"][1]].any())
    Q, p, A, b = _gpu(inp, dev, "Q", "p", "A", "b")
    with pytest.raises(RuntimeError, match=rf"Batch element {r['singular'][0]}\)"):
        L.torch_solve_qp_eqcon(Q, p, A, b)
    P.record(f"direct:{name}", "raises", 0.0, 1.0, batch_element=r["singular"][0])
    # ... and the next call on the same workspace is not disturbed by it
    ok = [i for i in range(r["B"]) if i != r["singular"][0]]
    sol = L.torch_solve_qp_eqcon(Q[ok], p[ok], A[ok], b[ok])
    assert bool(torch.isfinite(sol["x"]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# OptNet, equality-only branch
@pytest.mark.parametrize("name", _names("optnet"))
def test_optnet_against_the_oracle(dev, name):
    r = DT.ROW_BY_NAME[name]
    inp = DT.inputs(r)
    t64, t32 = _truths(r, inp)
    leaves = [t.clone().requires_grad_(True) for t in _gpu(inp, dev, "Q", "p", "A", "b")]
    x = L.OptNet(control=L.optnet_control())(*leaves, None, None)
    x.backward(inp["cot"].to(dev))
    torch.cuda.synchronize()
    hip = dict(x=x.detach(), **{k: t.grad for k, t in zip(GRADS6[:4], leaves)})
    bad = []
    res = _judge(r, hip, t32, t64, bad)
    if set(res) != {"x", "dQ", "dp", "dA", "db"}:
        bad.append(("compared", sorted(res)))
    assert not bad, (name, bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# SolveBoxQP / torch_solve_box_qp without any finite bound
def _hip_control(r, **extra):
    return L.box_qp_control(scale=r["ctl"].get("scale", True), **{k: r["ctl"][k] for k in ("launch_mode",) if k in r["ctl"]}, **extra)


@pytest.mark.parametrize("name", _names("layer0"))
def test_no_bound_layer_against_the_oracle(dev, cus, name):
    r = DT.ROW_BY_NAME[name]
    inp = DT.inputs(r)
    t64, t32 = _truths(r, inp)
    Q, p, A, b, cot = _gpu(inp, dev, "Q", "p", "A", "b", "cot")
    lb, ub = (t.to(dev) for t in DT._unbounded(inp["p"]))
    sync = r["ctl"].get("sync", True)
    case = f"direct:{name}"
    bad = []

    # ---- the functional solve: every output, the stats ----
    ctl = _hip_control(r)
    sol = L.torch_solve_box_qp(Q, p, A, b, lb, ub, ctl)
    st = sol["_stats"]
    P.record(case, "stats", 0.0, 1.0, cus=cus, tier=r["tier"], **{k: st[k] for k in ("iters", "any_lb", "any_ub", "linsolve_used", "mode_used", "loop_workgroups",
                                                            "factor_launches", "n_launch")})
    print(f"{case} stats: {st}")
    if not (sol["iter"] == 0 and st["any_lb"] == 0 and st["any_ub"] == 0 and st["linsolve_used"] == 1):
        bad.append(("stats", sol["iter"], st["any_lb"], st["any_ub"], st["linsolve_used"]))
    mode, lw = DT.TIERS[r["tier"]]
    if st["mode_used"] != mode or (st["loop_workgroups"] != lw if lw is not None else st["loop_workgroups"] <= 2):
        bad.append(("tier", r["tier"], st["mode_used"], st["loop_workgroups"]))
    if not (torch.is_tensor(sol["rho"]) is False and sol["rho"] == 0):
        bad.append(("rho", sol["rho"]))
    if ctl.get("rho") is not None:
        bad.append(("the functional solve wrote into its control", ctl.get("rho")))
    if bool(sol["u"].any()) or bool(sol["lams"].any()):
        bad.append(("u / lams not exactly zero", float(sol["u"].abs().max()), float(sol["lams"].abs().max())))
    if (sol["nus"] is None) != (r["m"] == 0):
        bad.append(("nus", r["m"]))
    _judge(r, {k: sol[k] for k in ("x", "z", "u", "lams", "nus") if sol[k] is not None}, t32, t64, bad)

    # ---- the module: forward, backward='fixed_point' and 'kkt' ----
    for tag in ("fp", "kkt"):
        mctl = _hip_control(r, backward="fixed_point" if tag == "fp" else "kkt", **({} if sync else dict(sync=False)))
        leaves = [None if t is None else t.clone().requires_grad_(True) for t in (Q, p, A, b)]
        x = L.SolveBoxQP(control=mctl)(*leaves, lb, ub)
        if not sync:
            L.synchronize()
        mst = SB.last_forward_status(dev)
        x.backward(cot)
        if not sync:
            L.synchronize()
        torch.cuda.synchronize()
        if mctl.get("rho") != 0 or torch.is_tensor(mctl.get("rho")):
            bad.append(("control['rho'] after the layer", tag, mctl.get("rho")))
        if not (mst["iters"] == 0 and mst["any_lb"] == 0 and mst["any_ub"] == 0 and mst["linsolve_used"] == 1):
            bad.append(("module stats", tag, mst))
        if sync and not torch.equal(x.detach(), sol["x"]):
            bad.append(("module x differs from the functional solve's", tag))
        hip = {f"{tag}.{k}": (None if t is None else t.grad) for k, t in zip(GRADS6[:4], leaves)}
        hip = {k: v for k, v in hip.items() if k in t64}
        if len(hip) != (4 if r["m"] else 2) or any(v is None for v in hip.values()):
            bad.append(("module gradients", tag, sorted(hip)))
        _judge(r, dict(hip, x=x.detach()), t32, t64, bad, tag="module." if tag == "fp" else "module_kkt.")

    # ---- the backward function with rho = 0, all six gradients, at the oracle's own solution ----
    pt = {k: (None if v is None else v.to(dev)) for k, v in DT.point(r, inp).items()}
    g = L.torch_solve_box_qp_grad(cot, pt["x"], pt["u"], pt["lams"], pt["nus"], Q, A, lb, ub, 0)
    torch.cuda.synchronize()
    if len(g) != 7 or g[6] is not None or [v is None for v in g[:6]] != [False, False, r["m"] == 0, r["m"] == 0, False, False]:
        bad.append(("direct: None pattern", [v is None for v in g]))
    hip = {f"direct.{k}": v for k, v in zip(GRADS6, g[:6]) if v is not None}
    res = _judge(r, hip, t32, t64, bad)
    if set(res) != {k for k in t64 if k.startswith("direct.")}:
        bad.append(("direct: compared", sorted(res)))
    assert not bad, (name, bad)
