"""Every row of tests/kkt_table.py on the GPU: backward='kkt' against the CPU oracle's KKT-system backward.  GPU only.

For each row: the row's entry point (SB._kkt_backward behind a symmetric forward, the functional torch_solve_box_qp_grad_kkt, or the
composition of torch ops) receives the synthetic primal-dual point of the row; the launch classes say which form ran (a Cholesky
row that fell back to the LU fails here) and the outputs that are None are the reference's.  Every gradient returned is compared
on the sampled problems with the oracle (oracle.boxqp_oracle.solve_box_qp_grad_kkt): truth in float64 on the same values, budget in
float32; float32 rows |hip - t64| <= R |t32 - t64| + F scale, float64 rows 1e-9 scale.  Rows that force a knob run once more with it
flipped and must differ observably (or, `same`, give the same bits).  Every ratio goes to the session's parity report, case
"kkt:<row>".  This module and tests/test_kkt_table.py are what pins backward='kkt'.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
import kkt_table as KT
import parity_report as P
import tier_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _call(r, gpu_pt, want=None):
    """The row's entry on the point (already on the GPU) under the current env -> ({name: gradient or None}, launches per class)."""
    _lib.profile(enable=True, reset=True)
    try:
        if r["entry"] == "chol":
            out = SB._kkt_backward(*gpu_pt, flags=KT.flags(r), linsolve=2, want=want)
        else:
            out = L.torch_solve_box_qp_grad_kkt(*gpu_pt)
        torch.cuda.synchronize()
        used = _lib.profile()
    finally:
        _lib.profile(enable=False)
    assert len(out) == 7 and out[6] is None
    return dict(zip(KT.GRADS, out[:6])), {k: v[1] for k, v in used.items()}


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(a[k], b[k])) for k in KT.GRADS)


@pytest.mark.parametrize("name", [r["name"] for r in KT.ROWS])
def test_kkt_backward_against_the_oracle(dev, cus, monkeypatch, name):
    r = KT.ROW_BY_NAME[name]
    B = T.batch(r, cus)
    pt = KT.point(r, B)
    idx = torch.tensor(T.sample(B))
    sub = tuple(None if t is None else t[idx] for t in pt)
    gpu_pt = tuple(None if t is None else t.to(dev) for t in pt)
    monkeypatch.setattr(SB, "_KKT_NATIVE", r["entry"] != "composed")
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    grads, prof = _call(r, gpu_pt)
    case = f"kkt:{name}"
    bad = []

    # ---- which form ran, which outputs exist ----
    ran = tuple(prof[c] for c in KT.PROF_CLASSES)
    P.record(case, "form", 0.0, 1.0, B=B, cus=cus, form=r["form"], prof=prof)
    if ran != KT.FORMS[r["form"]]:
        bad.append(("form", r["form"], dict(zip(KT.PROF_CLASSES, ran)), KT.FORMS[r["form"]]))
    for k, none in KT.none_pattern(r).items():
        if (grads[k] is None) != none:
            bad.append(("None pattern", k, grads[k] is None, none))

    # ---- every gradient on the sampled problems: truth in float64, budget in float32 ----
    t64 = KT.oracle(sub, torch.float64)
    t32 = KT.oracle(sub, torch.float32) if r["dtype"] == "f32" else None
    hip = {k: (None if v is None else v[idx.to(dev)].cpu()) for k, v in grads.items()}
    res = KT.compare(r, hip, t32, t64)
    if set(res) != {k for k in KT.GRADS if t64[k] is not None}:
        bad.append(("compared", sorted(res)))
    for k, rec in res.items():
        print(f"{case} {k}: err {rec['err']:.3e} budget {rec.get('budget', float('nan')):.3e} ratio {rec.get('ratio', float('nan')):.3g} "
              f"bar {rec['bar']:.3e} scale {rec['scale']:.3g} ok {rec['ok']}")
        P.record(case, k, rec["err"], rec["scale"], ratio=rec.get("ratio"), budget=rec.get("budget"), bar=rec["bar"],
                 R=r["R"], F=r["F"], dtype=r["dtype"])
        if not rec["ok"]:
            bad.append(("value", k, rec))

    # ---- subsets of `want`: what is still asked for keeps its bits, what is not is not returned ----
    if r["want"]:
        full = dict(dQ=True, dp=True, dA=r["m"] > 0, db=r["m"] > 0, dlb=True, dub=True)
        for sel in (dict(full, dlb=False, dub=False), dict({k: False for k in full}, dQ=True)):
            part, pprof = _call(r, gpu_pt, want=sel)
            for k in KT.GRADS:
                if sel[k] and not (part[k] is not None and torch.equal(part[k], grads[k])):
                    bad.append(("want subset changed", k, sel))
                if not sel[k] and part[k] is not None:
                    bad.append(("want subset returned", k, sel))
            if pprof != prof:
                bad.append(("want subset launches", pprof, prof))

    # ---- the forced knob must bite (or, `same`, must not change a bit) ----
    if r["flip"] is not None:
        for k in r["env"]:
            monkeypatch.delenv(k)
        for k, v in r["flip"].items():
            monkeypatch.setenv(k, v)
        alt, aprof = _call(r, gpu_pt)
        same_g = _same_bits(alt, grads)
        moved = sorted(k for k in prof if aprof.get(k) != prof[k])
        print(f"{case} flip {r['flip']}: same_grads {same_g} moved {moved}")
        P.record(case, "flip", 0.0, 1.0, same_grads=same_g, moved=moved, flip=r["flip"])
        if r["same"]:
            if not same_g:
                bad.append(("flip changed bits", r["flip"], moved))
        elif same_g and not moved:
            bad.append(("knob does not bite", r["env"], r["flip"]))
    assert not bad, (name, bad)
