"""Every row of tests/fp_table.py on the GPU: the fixed-point backward against the CPU oracle's, all six gradients.  GPU only.

For each row: the row's entry point (SB._fp_backward behind a symmetric forward, its two-phase form _fp_backward_prepare /
_fp_backward_run, the functional torch_solve_box_qp_grad, or that in two phases) receives the synthetic fixed point of the row,
whose free set has the size the row asks for; the launch classes say which form ran (a Cholesky row that fell back to the LU fails
here) and the outputs that are None are the reference's.  Every gradient is compared on the sampled problems with the oracle
(oracle.boxqp_oracle.solve_box_qp_grad): truth in float64 on the same values, budget in float32; float32 rows
|hip - t64| <= R |t32 - t64| + F scale, float64 rows 1e-9 scale.  Two-phase rows must give the bits of the one-call form on the same
point.  Rows that force a knob run once more with it flipped and must differ observably (or, `same`, give the same bits).  Every
ratio goes to the session's parity report, case "fp:<row>".  This module and tests/test_fp_table.py are what pins the fixed-point
backward at chosen free-set sizes; tests/tier_table.py reaches it behind a real forward solve.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
import fp_table as FT
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


def _full_want(r):
    return dict(dQ=True, dp=True, dA=r["m"] > 0, db=r["m"] > 0, dlb=True, dub=True)


def _call(r, gpu_pt, entry=None, want=None):
    """The entry on the point (already on the GPU) under the current env -> ({name: gradient or None}, launches per class)."""
    entry = entry or r["entry"]
    cot, rest = gpu_pt[0], gpu_pt[1:]
    want = want or _full_want(r)
    _lib.profile(enable=True, reset=True)
    try:
        if entry == "chol":
            out = SB._fp_backward(cot, *rest, want, linsolve=2)
        elif entry == "lu" and want == _full_want(r):
            out = L.torch_solve_box_qp_grad(cot, *rest)
        elif entry == "lu":
            out = SB._fp_backward(cot, *rest, want, linsolve=1)
        else:
            prep = SB._fp_backward_prepare(*rest, want, linsolve=2 if entry == "chol_pre" else 1, prefactor=True)
            out = SB._fp_backward_run(prep, cot)
        torch.cuda.synchronize()
        used = _lib.profile()
    finally:
        _lib.profile(enable=False)
    assert len(out) == 7 and out[6] is None
    return dict(zip(FT.GRADS, out[:6])), {k: v[1] for k, v in used.items()}


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(a[k], b[k])) for k in FT.GRADS)


@pytest.mark.parametrize("name", [r["name"] for r in FT.ROWS])
def test_fp_backward_against_the_oracle(dev, cus, monkeypatch, name):
    r = FT.ROW_BY_NAME[name]
    B = T.batch(r, cus)
    pt = FT.point(r, B)
    idx = torch.tensor(T.sample(B))
    sub = tuple(t[idx] if torch.is_tensor(t) else t for t in pt)
    gpu_pt = tuple(t.to(dev) if torch.is_tensor(t) else t for t in pt)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    grads, prof = _call(r, gpu_pt)
    case = f"fp:{name}"
    bad = []

    # ---- which form ran, which outputs exist ----
    ran = tuple(prof[c] for c in FT.PROF_CLASSES)
    P.record(case, "form", 0.0, 1.0, B=B, cus=cus, form=r["form"], prof=prof)
    if ran != FT.FORMS[r["form"]]:
        bad.append(("form", r["form"], dict(zip(FT.PROF_CLASSES, ran)), FT.FORMS[r["form"]]))
    for k, none in FT.none_pattern(r).items():
        if (grads[k] is None) != none:
            bad.append(("None pattern", k, grads[k] is None, none))

    # ---- all six gradients on the sampled problems: truth in float64, budget in float32 ----
    t64 = FT.oracle(sub, torch.float64)
    t32 = FT.oracle(sub, torch.float32) if r["dtype"] == "f32" else None
    hip = {k: (None if v is None else v[idx.to(dev)].cpu()) for k, v in grads.items()}
    res = FT.compare(r, hip, t32, t64)
    if set(res) != {k for k in FT.GRADS if t64[k] is not None}:
        bad.append(("compared", sorted(res)))
    for k, rec in res.items():
        print(f"{case} {k}: err {rec['err']:.3e} budget {rec.get('budget', float('nan')):.3e} ratio {rec.get('ratio', float('nan')):.3g} "
              f"bar {rec['bar']:.3e} scale {rec['scale']:.3g} ok {rec['ok']}")
        P.record(case, k, rec["err"], rec["scale"], ratio=rec.get("ratio"), budget=rec.get("budget"), bar=rec["bar"],
                 R=r["R"], F=r["F"], dtype=r["dtype"])
        if not rec["ok"]:
            bad.append(("value", k, rec))
    if name in FT.ZERO_BUDGET:          # (every free set empty: dv = 0 and dnu = 0 by algebra, in any precision)
        for k in ("dQ", "dp", "dA", "db"):
            if grads[k] is not None and bool(grads[k].any()):
                bad.append(("not exactly zero on an empty free set", k, float(grads[k].abs().max())))

    # ---- two phases: the bits of the one-call form on the same point ----
    if r["entry"].endswith("_pre"):
        one, oprof = _call(r, gpu_pt, entry=r["entry"][:-4])
        same_g = _same_bits(one, grads)
        print(f"{case} one call: same_grads {same_g}")
        P.record(case, "one_call", 0.0, 1.0, same_grads=same_g)
        if not same_g:
            bad.append(("two phases changed bits", [k for k in FT.GRADS if one[k] is not None and not torch.equal(one[k], grads[k])]))
        if tuple(oprof[c] for c in FT.PROF_CLASSES) != FT.FORMS[r["entry"][:-4]]:
            bad.append(("one-call form", oprof))

    # ---- subsets of `want`: what is still asked for keeps its bits, what is not is not returned ----
    if r["want"]:
        full = _full_want(r)
        for sel in (dict(full, dlb=False, dub=False), dict({k: False for k in full}, dQ=True), dict({k: False for k in full}, dub=True)):
            part, pprof = _call(r, gpu_pt, want=sel)
            for k in FT.GRADS:
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
        ahip = {k: (None if v is None else v[idx.to(dev)].cpu()) for k, v in alt.items()}
        ares = FT.compare(r, ahip, t32, t64)
        print(f"{case} flip {r['flip']}: same_grads {same_g} moved {moved} ratios "
              + " ".join(f"{k} {rec.get('ratio', float('nan')):.3g}" for k, rec in ares.items()))
        P.record(case, "flip", 0.0, 1.0, same_grads=same_g, moved=moved, flip=r["flip"],
                 ratios={k: rec.get("ratio") for k, rec in ares.items()})
        if r["same"]:
            if not same_g:
                bad.append(("flip changed bits", r["flip"], moved))
        elif same_g and not moved:
            bad.append(("knob does not bite", r["env"], r["flip"]))
    assert not bad, (name, bad)
