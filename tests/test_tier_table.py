"""CPU checks of tests/tier_table.py: the rows cover every schedule-selecting knob and both sides of every size threshold of the
selection code, the comparator of tests/test_gpu_tiers.py can see a one-tile error of 1e-4, and the build watches every
source file the library includes."""
import os
import re

import pytest
import torch

import tier_table as T
from lqp_py_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256          # (any count: the coverage below is about the expressions; the GPU module reads the real one)


def documented_knobs():
    """{name: default} of the LQP_* table in docs/KNOBS.md."""
    text = open(os.path.join(REPO, "docs", "KNOBS.md")).read()
    return {m.group(1): m.group(2).strip() for m in re.finditer(r"^\| `(LQP_\w+)` \| ([^|]+) \|", text, re.M)}


# documented in docs/KNOBS.md as "(Python)": read by the Python package, not by the library -- no entry in its knob list
PYTHON_KNOBS = {"LQP_UNROLL_EVENTS", "LQP_UNROLL_NATIVE", "LQP_UNROLL_SCALE_NATIVE"}


def library_knobs():
    """{name: default} of the LQP_KNOBS list in csrc/lqp_amd.hip, from which struct Knobs and read_knobs are generated."""
    text = open(os.path.join(_lib.CSRC, "lqp_amd.hip")).read()
    body = text[text.index("#define LQP_KNOBS(X)"):text.index("struct Knobs {")]
    return {m.group(2): m.group(3) for m in re.finditer(r'^\s*X\((\w+),\s*"(LQP_\w+)",\s*(-?\d+)\)', body, re.M)}


def test_knob_list_and_document_agree():
    """docs/KNOBS.md says it is generated from the library's knob list: the same names with the same defaults in both."""
    lib, doc = library_knobs(), documented_knobs()
    assert len(lib) > 40, "LQP_KNOBS list not parsed"
    assert PYTHON_KNOBS <= set(doc) and not PYTHON_KNOBS & set(lib)
    assert {k: v for k, v in doc.items() if k not in PYTHON_KNOBS} == lib


def uncovered_knobs(rows):
    knobs = documented_knobs()
    forced = {}
    for r in rows:
        for k, v in r["env"].items():
            if v != knobs.get(k):
                forced.setdefault(k, []).append(r["name"])
    return sorted(k for k in knobs if k not in T.NOT_A_TIER and k not in forced)


def uncovered_thresholds(rows):
    missing = []
    for what, (key, lo, hi) in T.THRESHOLDS.items():
        if key == "B":
            vals = {r["B"] for r in rows}
            ok = lo in vals and hi in vals
        else:
            get = (lambda r: r["n"] + r["m"]) if key == "N" else (lambda r: r[key])
            vals = {get(r) for r in rows}
            ok = lo in vals and hi in vals
        if not ok:
            missing.append(what)
    return missing


def test_rows_cover_every_knob_and_threshold():
    knobs = documented_knobs()
    assert len(knobs) > 40, "docs/KNOBS.md table not parsed"
    assert not set(T.NOT_A_TIER) - set(knobs), "exclusions that are not knobs"
    assert all(T.NOT_A_TIER.values())
    for r in T.ROWS:
        assert set(r["env"]) <= set(knobs) and set(r["flip"] or {}) <= set(knobs), r["name"]
        assert r["dtype"] in ("f32", "f64") and 0 < r["K"] <= T.K_EVENTS
        if r["K"] not in (T.K_DEFAULT, T.K_EVENTS):
            assert r["why"], r["name"]
        assert T.batch(r, CUS) >= 1 and "linsolve_used" in r["sig"], r["name"]
        assert r["R"] <= T.R_MAX and r["F"] <= T.F_MAX, r["name"]
        if (r["R"], r["F"]) != (T.R_DEFAULT, T.F_DEFAULT) or r["same"]:
            assert r["why"], (r["name"], "a raised bar or a same-bits flip needs its reason")
        if "n_factor" in r["sig"] and r["sig"]["n_factor"] > 1:
            assert r["K"] == T.K_EVENTS and r["ctl"].get("rho") in (0.01, 100.0), r["name"]
        if r["dtype"] == "f64":
            assert r["sig"]["linsolve_used"] == 1, r["name"]            # (the symmetric x-update is float32 only)
        if r["n"] + r["m"] >= 2048:
            assert T.batch(r, CUS) <= 2, r["name"]                       # (the oracle's cost)
    assert uncovered_knobs(T.ROWS) == []
    assert uncovered_thresholds(T.ROWS) == []
    # every symbolic batch size of the issue appears; both paths take launch mode 1 and 2 and sync True and False
    assert {"cus//4", "cus//4 + 1", "cus//2", "cus//2 + 1", "cus + 3"} <= {r["B"] for r in T.ROWS}
    for ls in (1, 2):
        rows = [r for r in T.ROWS if r["sig"]["linsolve_used"] == ls]
        assert {1, 2} <= {r["sig"].get("mode_used") for r in rows}, ls
        assert any(r["ctl"].get("sync") is False for r in rows), ls
    assert {0, 1, 16} <= {r["m"] for r in T.ROWS if r["sig"]["linsolve_used"] == 2}


def test_coverage_check_fails_without_its_rows():
    """The coverage check is not vacuous: without the only row that forces a knob, or without one side of a boundary pair, it fails."""
    knob_rows = {}
    for r in T.ROWS:
        for k in r["env"]:
            knob_rows.setdefault(k, []).append(r["name"])
    only = next(k for k, v in sorted(knob_rows.items()) if len(v) == 1 and k not in T.NOT_A_TIER)
    assert uncovered_knobs([r for r in T.ROWS if r["name"] != knob_rows[only][0]]) == [only]
    for what, (key, lo, hi) in T.THRESHOLDS.items():
        get = (lambda r: r["B"]) if key == "B" else (lambda r: r["n"] + r["m"]) if key == "N" else (lambda r: r[key])
        for side in (lo, hi):
            assert what in uncovered_thresholds([r for r in T.ROWS if get(r) != side]), (what, side)


SENS_ROWS = [r["name"] for r in T.ROWS if r["dtype"] == "f32" and r["n"] <= 513 and r["n"] >= 64]


@pytest.mark.parametrize("name", SENS_ROWS)
def test_comparator_sees_a_one_tile_error(name):
    """With the oracle's float32 solve standing in for the HIP one, the comparator passes; with the last (partial) diagonal 64-block
    of Q scaled by 1 + 1e-4 it fails, at the row's own R and F.  (Rows below n = 64 are left out: one tile is the whole matrix
    there, a relative error of Q is then mostly absorbed by the solve's scaling.)"""
    r = T.ROW_BY_NAME[name]
    B = T.batch(r, CUS)
    idx = T.sample(B)[:2]
    inp = T.inputs(r, B, idx)
    cot = torch.randn(len(idx), r["n"], 1, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    t64 = T.oracle(r, inp, torch.float64, cot)
    t32 = T.oracle(r, inp, torch.float32, cot)
    ok = T.compare(r, t32, t32, t64)
    ok.update(T.compare(r, t32["grads"], t32["grads"], t64["grads"], keys=T.GRADS))
    assert all(rec["ok"] for rec in ok.values()) and "dp" in ok, ok
    bad_inp = (T.perturb_last_block(inp[0]),) + tuple(inp[1:])
    wrong = T.oracle(r, bad_inp, torch.float32)
    res = T.compare(r, wrong, t32, t64)
    assert not all(rec["ok"] for rec in res.values()), {k: (v["err"], v["bar"]) for k, v in res.items()}


def _includes(path, seen):
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if p not in seen and os.path.exists(p):
            seen.add(p)
            _includes(p, seen)
    return seen


def test_build_watches_every_included_source():
    """A header of the library that the build does not watch leaves a stale liblqp_amd.so in use after an edit."""
    seen = _includes(os.path.join(_lib.CSRC, "lqp_amd.hip"), set())
    inside = {os.path.relpath(p, _lib.CSRC) for p in seen if p.startswith(_lib.CSRC + os.sep)}
    inside = {p for p in inside if not p.startswith("split" + os.sep)}     # (the split build's files: build_library adds them)
    assert "lqp_f16x2.hpp" in inside
    assert inside - set(_lib.SOURCES) == set()
