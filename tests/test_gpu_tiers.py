"""Every schedule of tests/tier_table.py on the GPU, against the CPU oracle at a pinned iteration count.  GPU only.

For each row: the HIP solve with eps_abs = eps_rel = 1e-12 and max_iters = K + 1 runs exactly K iterations and reports the
row's signature; the truth is the oracle in float64 on the same inputs, the budget the oracle in float32 (the same algorithm
with LAPACK's rounding).  Float32 rows: |hip - t64| <= R |t32 - t64| + F scale for x, z, u, lams, nus, rho and for the fixed-point
gradients of a fixed cotangent through the module (the prefactored backward of the row's forward); float64 rows: 1e-9 scale.
The rows with backward='kkt' compare their gradients with the oracle's KKT-system backward of the HIP solve's own x, lams, nus.
Rows that force a knob run once more with it flipped and must differ observably (or, `same`, give the same bits).  Every
ratio |hip - t64| / |t32 - t64| goes to the session's parity report (tests/parity_report.py), case "tier:<row>".
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import parity_report as P
import tier_table as T

pytestmark = pytest.mark.gpu
STAT_KEYS = ("n_launch", "factor_launches", "loop_workgroups", "mode_used", "linsolve_used")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cot(r, B, dt):
    g = torch.Generator().manual_seed(T.seed_of(r) + 1)
    return torch.randn(B, r["n"], 1, generator=g, dtype=torch.float64).to(dt)


def _run(r, dev, inp, cot):
    """Functional solve (all outputs, stats) and the module's forward + backward (gradients) of row r under the current env."""
    base = T.control(r)
    hip_ctl = O.make_control(**base, **{k: r["ctl"][k] for k in ("linsolve", "launch_mode") if k in r["ctl"]})
    args = [None if t is None else t.to(dev) for t in inp]
    _lib.profile(enable=True, reset=True)
    sol = L.torch_solve_box_qp(*args, dict(hip_ctl))
    Qg = args[0].clone().requires_grad_(True)
    pg = args[1].clone().requires_grad_(True)
    Ag = None if args[2] is None else args[2].clone().requires_grad_(True)
    bg = None if args[3] is None else args[3].clone().requires_grad_(True)
    mod_ctl = dict(hip_ctl, sync=r["ctl"].get("sync", True), backward=r["ctl"].get("backward", "fixed_point"))
    x = L.SolveBoxQP(control=mod_ctl)(Qg, pg, Ag, bg, args[4], args[5])
    mst = SB.last_forward_status(dev)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    prof = {k: v[1] for k, v in _lib.profile().items()}
    _lib.profile(enable=False)
    grads = dict(dQ=Qg.grad, dp=pg.grad, dA=None if Ag is None else Ag.grad, db=None if bg is None else bg.grad)
    return dict(sol=sol, stats=dict(sol["_stats"]), mstats=mst, xm=x.detach(), grads=grads, prof=prof)


def _pick(v, idx, dev):
    if torch.is_tensor(v) and v.dim() > 0:
        return v[idx.to(v.device)].detach().cpu()
    return v


@pytest.mark.parametrize("name", [r["name"] for r in T.ROWS])
def test_tier_against_the_pinned_oracle(dev, cus, monkeypatch, name):
    r = T.ROW_BY_NAME[name]
    B = T.batch(r, cus)
    K = r["K"]
    inp = T.inputs(r, B)
    dt = inp[1].dtype
    cot = _cot(r, B, dt)
    idx = torch.tensor(T.sample(B))
    sub = [None if t is None else t[idx] for t in inp]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    run = _run(r, dev, inp, cot)
    sol, st = run["sol"], run["stats"]
    case = f"tier:{name}"
    bad = []

    # ---- the oracle: truth in float64, budget in float32, both pinned to K iterations ----
    t64 = T.oracle(r, sub, torch.float64, cot[idx])
    t32 = T.oracle(r, sub, torch.float32, cot[idx]) if r["dtype"] == "f32" else None

    # ---- iteration count, signature, refactorisations ----
    P.record(case, "stats", 0.0, 1.0, B=B, cus=cus, **{k: st[k] for k in STAT_KEYS + ("n_factor", "iters")},
             t64_n_factor=t64["n_factor"], t32_n_factor=None if t32 is None else t32["n_factor"], prof=run["prof"])
    if sol["iter"] != K or run["mstats"]["iters"] != K:
        bad.append(("iter", sol["iter"], run["mstats"]["iters"], K))
    for k, v in r["sig"].items():
        if st[k] != v:
            bad.append(("sig", k, st[k], v))
    nf = [st["n_factor"], t64["n_factor"]] + ([] if t32 is None else [t32["n_factor"]])
    if len(set(nf)) != 1:
        bad.append(("n_factor hip / t64 / t32", nf))
    if not torch.equal(run["xm"], sol["x"]):
        bad.append(("module x differs from the functional solve's",))

    # ---- outputs and gradients on the sampled problems ----
    hip = {k: _pick(sol[k], idx, dev) for k in T.OUTPUTS}
    res = T.compare(r, hip, t32, t64)
    hg = {k: _pick(v, idx, dev) for k, v in run["grads"].items()}
    if r["ctl"].get("backward", "fixed_point") != "kkt":
        g32, g64 = None if t32 is None else t32["grads"], t64["grads"]
    else:
        # backward='kkt' is a function of the solve's own x, lams, nus: the oracle's KKT backward on the HIP solve's values, converted
        # exactly to float64 for the truth and evaluated in float32 for the budget (tests/test_gpu_kkt.py holds the KKT backward's own rows)
        def kkt(dtype):
            a = [None if t is None else t.to(dtype) for t in (cot[idx], hip["x"], hip["lams"], hip["nus"], sub[0], sub[2], sub[4], sub[5])]
            return dict(zip(T.GRADS, O.solve_box_qp_grad_kkt(*a)[:4]))
        g32, g64 = None if t32 is None else kkt(torch.float32), kkt(torch.float64)
    res.update({k: v for k, v in T.compare(r, hg, g32, g64, keys=T.GRADS).items()})
    for k, rec in res.items():
        P.record(case, k, rec["err"], rec["scale"], ratio=rec.get("ratio"), budget=rec.get("budget"), bar=rec["bar"],
                 R=r["R"], F=r["F"], dtype=r["dtype"])
        if not rec["ok"]:
            bad.append(("value", k, rec))

    # ---- the forced knob must bite (or, `same`, must not change a bit) ----
    if r["flip"] is not None:
        for k in r["env"]:
            monkeypatch.delenv(k)
        for k, v in r["flip"].items():
            monkeypatch.setenv(k, v)
        alt = _run(r, dev, inp, cot)
        same_x = torch.equal(alt["sol"]["x"], sol["x"])
        same_g = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(alt["grads"].values(), run["grads"].values()))
        moved = [k for k in STAT_KEYS if alt["stats"][k] != st[k]] + (["launch classes"] if alt["prof"] != run["prof"] else [])
        P.record(case, "flip", 0.0, 1.0, same_x=same_x, same_grads=same_g, moved=moved, flip=r["flip"],
                 **{f"flip_{k}": alt["stats"][k] for k in STAT_KEYS})
        if r["same"]:
            if not (same_x and same_g):
                bad.append(("flip changed bits", r["flip"], same_x, same_g))
        elif same_x and same_g and not moved:
            bad.append(("knob does not bite", r["env"], r["flip"]))
    assert not bad, (name, bad)
