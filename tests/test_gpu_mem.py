"""No result depends on what workspace and output memory held: every row of tests/mem_table.py under every mode of
tests/memharness.py.  GPU only.

One item is one run of a row's call (the callers of the row's home test: test_gpu_tiers._run, test_gpu_fp._call, ...) with
  fresh-XX  every torch.empty / torch.empty_like / _lib.workspace buffer filled with the byte XX (00 clean, FF NaN and -1, 7F huge and
            finite, 3C small and plausible), guards around each
  stale     the row's `before` call first (fresh-00), then the row on the SAME cached workspaces, left as they are; torch allocations
            filled with FF
and its inputs inside guarded copies.  The reference for bitwise equality is the row's own fresh-00 run, made once per row; the item
fresh-00 makes it again and must find the same bits: determinism is the precondition, a row that fails it fails.  Every mode asserts
  1. every returned tensor is finite and has the reference's bits (a gradient not asked for is None in both);
  2. every reported integer -- iteration counts, the forward's statistics, launch counts -- is the reference's, and the forward
     reports the row's own signature (no degraded schedule; a time-out raises);
  3. fresh-FF and stale: the row's bar against the float64 oracle, computed as its home test computes it (tier_table.compare with the
     row's R and F, 1e-9 of scale in float64; the each-rows the criterion of test_gpu_each.compare): no new tolerance;
  4. no guard byte changed; 5. no input byte changed; 6. what a returned view covers is finite (the padded tails of the combined
     z / u / lams / nus / rho buffer lie outside the views).
tests/test_mem_table.py holds the coverage rules and the harness's own tests; docs/WORKSPACE.md the audit of who writes what first.
"""
import contextlib

import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
import direct_table as DT
import each_table as ET
import fp_table as FT
import kkt_table as KT
import mem_table as MT
import memharness as H
import tier_table as T
import unroll_table as U
import test_gpu_direct as GD
import test_gpu_each as GE
import test_gpu_fp as GF
import test_gpu_kkt as GK
import test_gpu_tiers as GT
import test_gpu_unroll as GU

pytestmark = pytest.mark.gpu
GRADS6 = ("dQ", "dp", "dA", "db", "dlb", "dub")
STAT_KEYS = ("n_factor", "n_launch", "factor_launches", "loop_workgroups", "mode_used", "linsolve_used", "any_lb", "any_ub", "iters",
             "n_check", "rho_updated", "fail_index", "loop_kind")

_CPU = {}          # (table, row) -> the row's inputs on the host, built once
_REF = {}          # (table, row) -> its fresh-00 result (tensors on the host, integers)
_ORACLE = {}       # (table, row) -> the oracle's results, computed once


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    """the inputs, references and oracle results of every row go when the module is done (the largest rows hold 200 MB each)"""
    yield
    for cache in (_CPU, _REF, _ORACLE):
        cache.clear()
    H.release(_lib)


@contextlib.contextmanager
def _env(monkeypatch, env, **attrs):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        for k, v in attrs.items():
            m.setattr(SB, k, v)
        yield


def _cached(table, name, make):
    if (table, name) not in _CPU:
        _CPU[(table, name)] = make()
    return _CPU[(table, name)]


def _g(t, dev, off):
    return H.guarded(t.to(dev), offset_elems=off) if torch.is_tensor(t) else t


# ---------------------------------------------------------------------------------------------------------------------------------
# the callers: -> (tensors {name: tensor | None}, integers {name: int | float | list})
def _stats(prefix, st):
    return {f"{prefix}.{k}": st[k] for k in STAT_KEYS if k in st}


def _split_numbers(tensors, ints):
    """a rho that comes back as a python number (given and never adapted) is an integer-like: compared by value"""
    for k in [k for k, v in tensors.items() if v is not None and not torch.is_tensor(v)]:
        ints[k] = tensors.pop(k)
    return tensors, ints


def _call_tier(name, dev, cus, mp, off):
    r = T.ROW_BY_NAME[name]
    B = T.batch(r, cus)
    inp, cot = _cached("tier", name, lambda: (T.inputs(r, B), GT._cot(r, B, torch.float32 if r["dtype"] == "f32" else torch.float64)))
    with _env(mp, r["env"]):
        run = GT._run(r, dev, [_g(t, dev, off) for t in inp], _g(cot, dev, off))
    sol = run["sol"]
    tensors = {k: sol[k] for k in T.OUTPUTS}
    tensors.update(xm=run["xm"], **run["grads"])
    ints = dict(iter=sol["iter"], **_stats("stats", run["stats"]), **_stats("module", run["mstats"]))
    sig = {k: (run["stats"][k], v) for k, v in r["sig"].items() if run["stats"][k] != v}
    assert not sig and sol["iter"] == r["K"] == run["mstats"]["iters"], (name, "signature / iterations", sig, sol["iter"], run["mstats"]["iters"])
    return _split_numbers(tensors, ints)


def _want_subsets(r):
    full = GF._full_want(r)
    return (dict(full, dlb=False, dub=False), dict({k: False for k in full}, dQ=True), dict({k: False for k in full}, dub=True))


def _call_backward(table):
    tab, mod = (FT, GF) if table == "fp" else (KT, GK)

    def call(name, dev, cus, mp, off):
        r = tab.ROW_BY_NAME[name]
        B = T.batch(r, cus)
        pt = _cached(table, name, lambda: tab.point(r, B))
        gpu_pt = tuple(_g(t, dev, off) for t in pt)
        attrs = dict(_KKT_NATIVE=r["entry"] != "composed") if table == "kkt" else {}
        with _env(mp, r["env"], **attrs):
            grads, prof = mod._call(r, gpu_pt)
            tensors = dict(grads)
            ints = {f"launches.{c}": prof[c] for c in tab.PROF_CLASSES}
            form = tuple(prof[c] for c in tab.PROF_CLASSES)
            assert form == tab.FORMS[r["form"]], (name, "form", form)
            if r["want"]:
                # an output that is not asked for is not returned (the kernels get a null pointer), one that is asked for is written
                # whole: the bits of the full call, whatever its memory held before
                for i, sel in enumerate(_want_subsets(r)[:3 if table == "fp" else 2]):
                    part, pprof = mod._call(r, gpu_pt, want=sel)
                    assert pprof == prof, (name, "want subset launches", sel)
                    for k in GRADS6:
                        assert (part[k] is not None) == bool(sel[k] and grads[k] is not None), (name, "want subset returned", k, sel)
                        tensors[f"{k}@want{i}"] = part[k]
                        if part[k] is not None:
                            assert H.same_bits(part[k], grads[k]), (name, "want subset changed", k, sel)
        return tensors, ints
    return call


def _call_unroll(name, dev, cus, mp, off):
    r = U.ROW_BY_NAME[name]
    B, dt = U.batch(r, cus), U.dtype_of(r)
    inp, cot = _cached("unroll", name, lambda: (U.inputs(r, B), U.cotangent(r, B).to(dt)))
    with _env(mp, r["env"]):
        hip, prof = GU._backward(r, dev, [_g(t, dev, off) for t in inp], _g(cot, dev, off), GU._hip_control(r, B, dev, dt))
    exp = r["exp"]
    assert (prof["unroll_backward"], prof["unroll_scaling"]) == (exp["ub"], exp["us"]), (name, "launches", prof["unroll_backward"], prof["unroll_scaling"])
    return dict(hip), {"launches.unroll_backward": prof["unroll_backward"], "launches.unroll_scaling": prof["unroll_scaling"]}


def _call_direct(name, dev, cus, mp, off):
    r = DT.ROW_BY_NAME[name]
    inp = _cached("direct", name, lambda: DT.inputs(r))
    fam = r["family"]
    g = {k: (_g(v, dev, off) if k != "point" else v) for k, v in inp.items()}
    tensors, ints = {}, {}
    with _env(mp, r["env"]):
        if fam == "solve":
            (xa, x1, x2), rhs, before = GD._solve_once(r, g, dev)
            assert torch.equal(rhs, before) and H.same_bits(x1, x2) and H.same_bits(xa, x1), (name, "solve: rhs / repeated / repacked")
            tensors.update(x=x1)
        elif fam == "lulayer":
            M, rhs, gb = g["M"], DT.shape_rhs(r, g["base"]), DT.shape_rhs(r, g["gbase"])
            for tag in ("cached", "uncached"):
                Mg, rg = M.clone().requires_grad_(True), rhs.clone().requires_grad_(True)
                x = L.TorchLU(A=M)(Mg, rg) if tag == "cached" else L.TorchLULayer.apply(Mg, rg)
                x.backward(gb)
                tensors.update({f"{tag}.x": x.detach(), f"{tag}.dA": Mg.grad, f"{tag}.db": rg.grad})
        elif fam in ("eqcon", "uncon"):
            pt = {k: (None if v is None else v.to(dev)) for k, v in DT.point(r, inp).items()}
            if fam == "eqcon":
                sol = L.torch_solve_qp_eqcon(g["Q"], g["p"], g["A"], g["b"])
                gr = L.torch_solve_qp_eqcon_grad(g["cot"], pt["x"], pt["nus"], g["Q"], g["A"])
                tensors.update(x=sol["x"], nus=sol["nus"], **dict(zip(GRADS6[:4], gr)))
            else:
                sol = L.torch_solve_qp_uncon(g["Q"], g["p"])
                tensors.update(x=sol["x"], **dict(zip(GRADS6[:2], L.torch_solve_qp_uncon_grad(g["cot"], pt["x"], g["Q"]))))
        elif fam == "optnet":
            leaves = [g[k].clone().requires_grad_(True) for k in ("Q", "p", "A", "b")]
            x = L.OptNet(control=L.optnet_control())(*leaves, None, None)
            x.backward(g["cot"])
            tensors.update(x=x.detach(), **{k: t.grad for k, t in zip(GRADS6[:4], leaves)})
        else:
            assert fam == "layer0"
            Q, p, A, b, cot = (g[k] for k in ("Q", "p", "A", "b", "cot"))
            lb, ub = (_g(t, dev, off) for t in DT._unbounded(inp["p"]))
            sync = r["ctl"].get("sync", True)
            sol = L.torch_solve_box_qp(Q, p, A, b, lb, ub, GD._hip_control(r))
            st = sol["_stats"]
            assert sol["iter"] == 0 and st["any_lb"] == 0 and st["any_ub"] == 0 and st["linsolve_used"] == 1, (name, st)
            mode, lw = DT.TIERS[r["tier"]]
            assert st["mode_used"] == mode and (st["loop_workgroups"] == lw if lw is not None else st["loop_workgroups"] > 2), (name, "tier", st)
            tensors.update({k: sol[k] for k in ("x", "z", "u", "lams", "nus")})
            ints.update(iter=sol["iter"], rho=sol["rho"], **_stats("stats", st))
            for tag in ("fp", "kkt"):
                mctl = GD._hip_control(r, backward="fixed_point" if tag == "fp" else "kkt", **({} if sync else dict(sync=False)))
                leaves = [None if t is None else t.clone().requires_grad_(True) for t in (Q, p, A, b)]
                x = L.SolveBoxQP(control=mctl)(*leaves, lb, ub)
                if not sync:
                    L.synchronize()
                ints.update(_stats(f"module_{tag}", SB.last_forward_status(dev)))
                x.backward(cot)
                if not sync:
                    L.synchronize()
                tensors.update({f"module_{tag}.x": x.detach(), **{f"{tag}.{k}": (None if t is None else t.grad) for k, t in zip(GRADS6[:4], leaves)}})
            pt = {k: (None if v is None else v.to(dev)) for k, v in DT.point(r, inp).items()}
            gr = L.torch_solve_box_qp_grad(cot, pt["x"], pt["u"], pt["lams"], pt["nus"], Q, A, lb, ub, 0)
            tensors.update({f"direct.{k}": v for k, v in zip(GRADS6, gr[:6])})
        torch.cuda.synchronize()
    return tensors, ints


def _call_each(name, dev, cus, mp, off):
    row = ET.ROWS[name]
    extra, env, sync_split, _problems, _kind = MT.EACH_CALL[name]
    qp = _cached("each", name, lambda: ET.inputs(row, row["dtype"]))
    with _env(mp, env, **({} if sync_split is None else dict(_SYNC_SPLIT=sync_split))):
        sol = L.torch_solve_box_qp(*(_g(t, dev, off) for t in qp), GE.gpu_control(row, **extra))
        st = SB.last_forward_status(dev)
    tensors = {k: sol[k] for k in GE.KEYS + ("iters",)}
    ints = dict(iter=sol["iter"], **_stats("stats", sol["_stats"]), **_stats("status", st), loop_workgroups_per_qp=st["loop_workgroups_per_qp"])
    return _split_numbers(tensors, ints)


CALL = {"tier": _call_tier, "fp": _call_backward("fp"), "kkt": _call_backward("kkt"), "unroll": _call_unroll, "direct": _call_direct,
        "each": _call_each}


# ---------------------------------------------------------------------------------------------------------------------------------
# the rows' own bars against the float64 oracle, as their home tests compute them: -> the list of failures
def _failures(res, tag=""):
    return [(tag + k, rec) for k, rec in res.items() if not rec["ok"]]


def _bar_tier(name, out, cus):
    r = T.ROW_BY_NAME[name]
    B = T.batch(r, cus)
    inp, cot = _CPU[("tier", name)]
    idx = torch.tensor(T.sample(B))
    sub = [None if t is None else t[idx] for t in inp]
    if ("tier", name) not in _ORACLE:
        _ORACLE[("tier", name)] = (T.oracle(r, sub, torch.float64, cot[idx]), T.oracle(r, sub, torch.float32, cot[idx]) if r["dtype"] == "f32" else None)
    t64, t32 = _ORACLE[("tier", name)]
    pick = lambda v: v[idx] if torch.is_tensor(v) and v.dim() > 0 else v
    hip = {k: pick(out[k]) for k in T.OUTPUTS}
    bad = _failures(T.compare(r, hip, t32, t64))
    nf = {out["stats.n_factor"], t64["n_factor"]} | (set() if t32 is None else {t32["n_factor"]})
    if len(nf) != 1:
        bad.append(("n_factor hip / t64 / t32", sorted(nf)))
    assert r["ctl"].get("backward", "fixed_point") != "kkt"          # (tests/kkt_table.py's rows hold the KKT backward here)
    hg = {k: pick(out[k]) for k in T.GRADS}
    res = T.compare(r, hg, None if t32 is None else t32["grads"], t64["grads"], keys=T.GRADS)
    if set(res) != {k for k in T.GRADS if t64["grads"][k] is not None}:
        bad.append(("gradients compared", sorted(res)))
    return bad + _failures(res)


def _bar_backward(table):
    tab = FT if table == "fp" else KT

    def bar(name, out, cus):
        r = tab.ROW_BY_NAME[name]
        B = T.batch(r, cus)
        idx = torch.tensor(T.sample(B))
        sub = tuple(t[idx] if torch.is_tensor(t) else t for t in _CPU[(table, name)])
        if (table, name) not in _ORACLE:
            _ORACLE[(table, name)] = (tab.oracle(sub, torch.float64), tab.oracle(sub, torch.float32) if r["dtype"] == "f32" else None)
        t64, t32 = _ORACLE[(table, name)]
        hip = {k: (None if out[k] is None else out[k][idx]) for k in GRADS6}
        res = tab.compare(r, hip, t32, t64)
        bad = [] if set(res) == {k for k in GRADS6 if t64[k] is not None} else [("compared", sorted(res))]
        bad += [("None pattern", k) for k, none in tab.none_pattern(r).items() if (out[k] is None) != none]
        return bad + _failures(res)
    return bar


def _bar_unroll(name, out, cus):
    r = U.ROW_BY_NAME[name]
    B = U.batch(r, cus)
    inp, cot = _CPU[("unroll", name)]
    idx = U.sample(B)
    it = torch.tensor(idx)
    sub = [None if t is None else t[it] for t in inp]
    if ("unroll", name) not in _ORACLE:
        _ORACLE[("unroll", name)] = (U.tape(r, sub, torch.float64, cot[it], B, idx)[0],
                                     U.tape(r, sub, torch.float32, cot[it], B, idx)[0] if r["dtype"] == "f32" else None)
    t64, t32 = _ORACLE[("unroll", name)]
    pick = {k: (None if out[k] is None else out[k][it]) for k in ("x",) + U.GRADS}
    res = U.judge(r, pick, t32, t64, U.tie_mask(sub))
    missing = [k for k in U.KEYS if k not in res and not (r["m"] == 0 and k in ("dA", "db"))]
    return ([("outputs not compared", missing)] if missing else []) + _failures(res)


def _bar_direct(name, out, cus):
    r = DT.ROW_BY_NAME[name]
    inp = _CPU[("direct", name)]
    if ("direct", name) not in _ORACLE:
        _ORACLE[("direct", name)] = GD._truths(r, inp)
    t64, t32 = _ORACLE[("direct", name)]
    fam = r["family"]
    if fam == "lulayer":
        groups = [(tag + ".", {k: out[f"{tag}.{k}"] for k in ("x", "dA", "db")}) for tag in ("cached", "uncached")]
    elif fam == "layer0":
        groups = [("", {k: out[k] for k in ("x", "z", "u", "lams", "nus") if out[k] is not None})]
        for tag in ("fp", "kkt"):
            groups.append((f"module_{tag}.", dict({k: v for k, v in out.items() if k.startswith(tag + ".") and v is not None}, x=out[f"module_{tag}.x"])))
        groups.append(("", {k: v for k, v in out.items() if k.startswith("direct.") and v is not None}))
    else:
        groups = [("", {k: v for k, v in out.items() if v is not None})]
    bad, seen = [], set()
    for tag, hip in groups:
        res = DT.compare(r, hip, t32, t64, keys=tuple(k for k in t64 if k in hip))
        seen |= set(res)
        bad += _failures(res, tag)
    if seen != set(t64) - ({"nus"} if fam == "optnet" else set()):          # (the OptNet layer returns x alone)
        bad.append(("compared", sorted(seen), sorted(t64)))
    return bad


def _bar_each(name, out, cus):
    row = ET.ROWS[name]
    problems = MT.EACH_CALL[name][3]
    bad = []
    if out["iters"].tolist() != row["iters"] or out["iter"] != max(row["iters"]):
        bad.append(("iterations per problem", out["iters"].tolist(), row["iters"], out["iter"]))
    sol = dict(out)
    if problems == "done":                      # (test_host_driven_persistent_chunks: the problems that never become optimal are not compared)
        done = [b for b in range(row["B"]) if b not in row["never"]]
        sol = {k: (out[k] if not torch.is_tensor(out[k]) else out[k][done]) for k in ("x", "z", "u", "lams", "nus")}
        return bad + GE.compare(name, sol, problems=done, what=("x", "z", "u", "lams", "nus"))
    return bad + GE.compare(name, sol)


BAR = {"tier": _bar_tier, "fp": _bar_backward("fp"), "kkt": _bar_backward("kkt"), "unroll": _bar_unroll, "direct": _bar_direct,
       "each": _bar_each}


# ---------------------------------------------------------------------------------------------------------------------------------
def _host(tensors):
    return {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in tensors.items()}


def _run(table, name, dev, cus, mp, fill, off=0, keep_workspaces=False):
    """One run of the row under `fill` -> (tensors on the host, integers, what the guards and the inputs show, the harness's counters)"""
    if not keep_workspaces:
        H.release(_lib)
    with H.controlled_memory(mp, fill) as st:
        tensors, ints = CALL[table](name, dev, cus, mp, off)
        torch.cuda.synchronize()
        assert len(H._records) > len(H._inputs), (table, name, "no torch.empty of the call went through the harness")
        assert not MT.tags(table, name) or st["ws_created"] + st["ws_reused"] + st["ws_grown"] > 0, (table, name, "no workspace asked for")
        counters = {k: (sorted(v) if isinstance(v, (set, list)) else v) for k, v in st.items() if k != "active"}
    found = dict(guards=H.check_guards(), inputs=H.check_inputs_untouched())
    out = _host(tensors)
    if keep_workspaces:
        H.forget()
    else:
        H.release(_lib)
    return out, ints, found, counters


def _reference(table, name, dev, cus, mp):
    if (table, name) not in _REF:
        out, ints, found, _ = _run(table, name, dev, cus, mp, 0x00)
        assert not found["guards"] and not found["inputs"], (name, "fresh-00 reference", found)
        _REF[(table, name)] = (out, ints)
    return _REF[(table, name)]


def _against_reference(out, ints, ref, bad):
    rt, ri = ref
    if set(out) != set(rt) or set(ints) != set(ri):
        bad.append(("outputs", sorted(set(out) ^ set(rt)), sorted(set(ints) ^ set(ri))))
    for k, v in out.items():
        if v is not None and v.is_floating_point() and not bool(torch.isfinite(v).all()):
            bad.append(("not finite", k, int((~torch.isfinite(v)).sum())))
        if k in rt and not H.same_bits(v, rt[k]):
            both = v is not None and rt[k] is not None and v.shape == rt[k].shape
            bad.append(("bits differ from the fresh-00 run", k, float((v.double() - rt[k].double()).abs().nan_to_num(nan=float("inf")).max()) if both else None))
    for k, v in ints.items():
        if k in ri and ri[k] != v:
            bad.append(("integer differs from the fresh-00 run", k, v, ri[k]))


@pytest.mark.parametrize("mode", MT.MODES)
@pytest.mark.parametrize("rid", [r["id"] for r in MT.ROWS])
def test_result_does_not_depend_on_memory(dev, cus, monkeypatch, rid, mode):
    row = MT.ROW_BY_ID[rid]
    table, name = row["table"], row["row"]
    ref = _reference(table, name, dev, cus, monkeypatch)
    bad = []
    if mode == "stale":
        bt, bn = row["before"]
        H.release(_lib)
        with H.controlled_memory(monkeypatch, 0x00):
            CALL[bt](bn, dev, cus, monkeypatch, 0)
            torch.cuda.synchronize()
        found_b = dict(guards=H.check_guards(), inputs=H.check_inputs_untouched())
        H.forget()                                                                      # (the cached workspaces stay)
        if found_b["guards"] or found_b["inputs"]:
            bad.append(("the `before` call", found_b))
        out, ints, found, counters = _run(table, name, dev, cus, monkeypatch, None, keep_workspaces=True)
        H.release(_lib)
        shared = MT.tags(table, name) & MT.tags(bt, bn)
        if not shared <= set(counters["tags_stale"]) or shared & set(counters["tags_created"]) or (counters["ws_grown"] > 0) != (rid in MT.GROWS):
            bad.append(("the row did not run in what its `before` left", sorted(shared), counters))
    else:
        out, ints, found, counters = _run(table, name, dev, cus, monkeypatch, H.FILLS[mode.split("-")[1]])
    print(rid, mode, counters, {k: v for k, v in ints.items() if k.startswith(("iter", "stats.n_", "launches"))})
    _against_reference(out, ints, ref, bad)
    if mode in ("fresh-FF", "stale"):
        bad += [("the row's bar against the oracle",) + tuple(b) for b in BAR[table](name, dict(out, **ints), cus)]
    if found["guards"]:
        bad.append(("a guard byte changed", found["guards"]))
    if found["inputs"]:
        bad.append(("an input changed", found["inputs"]))
    if counters["unguarded"]:
        bad.append(("allocations the harness could not guard", counters["unguarded"]))
    assert not bad, (rid, mode, bad)


@pytest.mark.parametrize("table,name", MT.MISALIGNED, ids=[f"{t}:{n}" for t, n in MT.MISALIGNED])
def test_inputs_at_an_element_aligned_address(dev, cus, monkeypatch, table, name):
    """Q, p, A, ... as slices of one flat vector, flat[1:1 + numel].view(shape): the bits of the aligned call, within the row's bar.
    (_lib.norm / _lib.c copy such a tensor to a 16-byte aligned address, include/lqp_amd.h asks for one: docs/WORKSPACE.md.)"""
    ref = _reference(table, name, dev, cus, monkeypatch)
    out, ints, found, counters = _run(table, name, dev, cus, monkeypatch, 0xFF, off=1)
    bad = []
    _against_reference(out, ints, ref, bad)
    bad += [("the row's bar against the oracle",) + tuple(b) for b in BAR[table](name, dict(out, **ints), cus)]
    assert not bad and not found["guards"] and not found["inputs"], (table, name, bad, found)


def test_the_harness_on_device_memory(dev, monkeypatch):
    """What tests/test_mem_table.py checks on CPU tensors, on the GPU: the fill lands, a store one element past a payload is reported."""
    H.release(_lib)
    with H.controlled_memory(monkeypatch, 0x7F):
        t = torch.empty((5, 3), dtype=torch.float32, device=dev)
        ws = _lib.workspace(dev, 1000, "fwd")
        e = torch.empty_like(t)
    for v in (t, ws, e):
        assert v.is_cuda and v.data_ptr() % 256 == 0 and bool((v.view(-1).view(torch.uint8) == 0x7F).all())
    assert H.check_guards() == []
    torch.as_strided(t.view(-1), (16,), (1,))[15] = 0.0
    found = H.check_guards()
    assert len(found) == 1 and found[0]["side"] == "back" and found[0]["first"] == 0 and found[0]["count"] == 4, found
    g = H.guarded(torch.ones(7, device=dev), offset_elems=1)
    assert g.data_ptr() % 16 == 4 and _lib.norm(g, torch.float32).data_ptr() % 16 == 0 and H.check_inputs_untouched() == []
    g[3] = 2.0
    assert len(H.check_inputs_untouched()) == 1
    H.release(_lib)


def test_pinned_allocations_are_filled_and_reports_still_arrive(dev, monkeypatch):
    H.release(_lib)
    with H.controlled_memory(monkeypatch, 0x3C):
        t = torch.empty(64, dtype=torch.int32, pin_memory=True)
        assert t.is_pinned() and bool((t == 0x3C3C3C3C).all())
        with _lib._pinned_lock:
            _lib._pinned_free.pop(23, None)
        rep = _lib.host_report(23)               # (a fresh slab of the pool: filled; the library sets the words to -1 itself)
        assert rep.is_pinned() and bool((rep == 0x3C3C3C3C).all())
        _lib.report_done(rep)
    H.release(_lib)
