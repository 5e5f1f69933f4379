"""Every row of tests/unroll_table.py on the GPU: the gradients of ``unroll=True`` against autograd through the CPU oracle's own loop
at a pinned iteration count.  GPU only.

For each row: the module with unroll=True, eps_abs = eps_rel = 1e-12 and max_iters = K + 1, forward and backward of a fixed
cotangent; the truth is the oracle's tape in float64 on the same inputs (oracle.boxqp_oracle.unrolled_grad), the budget the same
tape in float32.  Float32 rows: |hip - t64| <= R |t32 - t64| + F scale for x, dQ, dp, dA, db, dlb, dub; float64 rows: 1e-9 scale
(tier_table.compare).  At lb == ub entries dlb + dub is compared, everywhere else dlb and dub by themselves (unroll_table.judge).
Also per row: the functional solve under the same control (and LQP_EQ_IN_LOOP=0: the unroll forward leaves the equality-corrected
inverse in its workspace for the sweep, which is that knob's schedule of the forward) ran exactly K iterations on the expected
x-update with the expected number of factorisations -- the oracle's tapes too --, the module's x has its bits, every gradient is
finite, the profile shows the row's launch counts, and (symmetric rows, 128 < n <= 512) LQP_UNROLL_SPLIT=0 changes gradient bits
exactly where the split sweep
runs.  Every ratio goes to the session's parity report, case "unroll:<row>".
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import parity_report as P
import unroll_table as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _hip_control(r, B, dev, dt):
    ctl = U.make_control(r, B, dtype=dt)
    if torch.is_tensor(ctl.get("beta")):
        ctl["beta"] = ctl["beta"].to(dev)
    if "linsolve" in r["ctl"]:
        ctl["linsolve"] = r["ctl"]["linsolve"]
    return ctl


def _backward(r, dev, inp, cot, ctl):
    """Forward + backward of the module with unroll=True under the current env: -> ({x, dQ ... dub}, launch counts)."""
    leaves = [None if t is None else t.to(dev).requires_grad_(True) for t in inp]
    _lib.profile(enable=True, reset=True)
    x = L.SolveBoxQP(control=dict(ctl, unroll=True))(*leaves)
    assert torch.is_tensor(x)
    x.backward(cot.to(dev))
    torch.cuda.synchronize()
    prof = {k: v[1] for k, v in _lib.profile().items()}
    _lib.profile(enable=False)
    out = dict(zip(U.GRADS, (None if t is None else t.grad for t in leaves)), x=x.detach())
    return out, prof


@pytest.mark.parametrize("name", [r["name"] for r in U.ROWS])
def test_unroll_row_against_the_oracle_tape(dev, cus, monkeypatch, name):
    r = U.ROW_BY_NAME[name]
    B, K, dt = U.batch(r, cus), r["K"], U.dtype_of(r)
    inp = U.inputs(r, B)
    cot = U.cotangent(r, B).to(dt)
    idx = U.sample(B)
    it = torch.tensor(idx)
    sub = [None if t is None else t[it] for t in inp]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    ctl = _hip_control(r, B, dev, dt)
    hip, prof = _backward(r, dev, inp, cot, ctl)
    # (the unroll forward keeps the equality-corrected inverse in its workspace for the sweep: the schedule of LQP_EQ_IN_LOOP=0)
    monkeypatch.setenv("LQP_EQ_IN_LOOP", "0")
    sol = L.torch_solve_box_qp(*[None if t is None else t.to(dev) for t in inp], dict(ctl, unroll=False))
    monkeypatch.delenv("LQP_EQ_IN_LOOP")
    st = sol["_stats"]
    case, bad, exp = f"unroll:{name}", [], r["exp"]

    # ---- the oracle's tapes: truth in float64, budget in float32, both pinned to K iterations ----
    t64, _ = U.tape(r, sub, torch.float64, cot[it], B, idx)
    t32 = U.tape(r, sub, torch.float32, cot[it], B, idx)[0] if r["dtype"] == "f32" else None

    # ---- iterations, x-update, factorisations, launches ----
    P.record(case, "stats", 0.0, 1.0, B=B, cus=cus, iters=sol["iter"], linsolve_used=st["linsolve_used"], n_factor=st["n_factor"],
             t64_n_factor=t64["n_factor"], t32_n_factor=None if t32 is None else t32["n_factor"],
             unroll_backward=prof["unroll_backward"], unroll_scaling=prof["unroll_scaling"], family=r["family"])
    if sol["iter"] != K or st["iters"] != K:
        bad.append(("iter", sol["iter"], st["iters"], K))
    if st["linsolve_used"] != exp["linsolve_used"] and r["family"] != "taped":
        bad.append(("linsolve_used", st["linsolve_used"], exp["linsolve_used"]))
    nf = [st["n_factor"], t64["n_factor"]] + ([] if t32 is None else [t32["n_factor"]])
    if set(nf) != {exp["n_factor"]}:
        bad.append(("n_factor hip / t64 / t32, expected", nf, exp["n_factor"]))
    if (prof["unroll_backward"], prof["unroll_scaling"]) != (exp["ub"], exp["us"]):
        bad.append(("launches unroll_backward / unroll_scaling", prof["unroll_backward"], prof["unroll_scaling"], exp["ub"], exp["us"]))
    if r["family"] != "taped" and not torch.equal(hip["x"], sol["x"]):
        bad.append(("module x differs from the functional solve's",))
    for k, v in hip.items():
        if v is not None and not bool(torch.isfinite(v).all()):
            bad.append(("not finite", k))

    # ---- x and the six gradients on the sampled problems ----
    pick = {k: (None if v is None else v[it.to(v.device)]) for k, v in hip.items()}
    res = U.judge(r, pick, t32, t64, U.tie_mask(sub))
    for k, rec in res.items():
        print(f"{case} {k}: err {rec['err']:.3e} budget {rec.get('budget')} ratio {rec.get('ratio')} bar {rec['bar']:.3e} ok {rec['ok']}")
        P.record(case, k, rec["err"], rec["scale"], ratio=rec.get("ratio"), budget=rec.get("budget"), bar=rec["bar"],
                 R=r["R"], F=r["F"], dtype=r["dtype"], family=r["family"])
        if not rec["ok"]:
            bad.append(("value", k, rec))
    missing = [k for k in U.KEYS if k not in res and not (r["m"] == 0 and k in ("dA", "db"))]
    if missing:
        bad.append(("outputs not compared", missing))

    # ---- which sweep ran: LQP_UNROLL_SPLIT=0 changes bits where the split sweep runs, and only there ----
    if r["split"] is not None:
        monkeypatch.setenv("LQP_UNROLL_SPLIT", "0")
        alt, aprof = _backward(r, dev, inp, cot, ctl)
        same = all((a is None and b is None) or torch.equal(a, b) for a, b in zip(alt.values(), hip.values()))
        P.record(case, "split", 0.0, 1.0, expected_split=r["split"], same_bits_without=same)
        if same == r["split"]:
            bad.append(("split sweep expected / LQP_UNROLL_SPLIT=0 gives the same bits", r["split"], same))
    assert not bad, (name, bad)
