"""tests/memharness.py tested on CPU tensors, and the coverage rules of tests/mem_table.py.  No GPU needed."""
import os

import pytest
import torch

from lqp_py_amd import _lib
import fp_table as FT
import kkt_table as KT
import mem_table as MT
import memharness as H
import unroll_table as U

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _clean():
    H.release(_lib)
    yield
    H.release(_lib)


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness
@pytest.mark.parametrize("fill", sorted(H.FILLS.values()))
def test_fills_land(monkeypatch, fill):
    with H.controlled_memory(monkeypatch, fill):
        a = torch.empty((3, 5, 1), dtype=torch.float32)
        b = torch.empty(7, dtype=torch.float64)
        c = torch.empty_like(a)
        d = torch.empty(3, 2, dtype=torch.int32)
        e = torch.empty(0)
        h = torch.empty((2, 3), dtype=torch.float16)
        ws = _lib.workspace(CPU, 1000, "fwd", stream=0)
    assert torch.empty is H._real_empty and torch.empty_like is H._real_empty_like      # (put back on exit)
    assert a.shape == (3, 5, 1) and b.shape == (7,) and c.shape == a.shape and c.dtype == a.dtype and e.numel() == 0
    for t in (a, b, c, d, h, ws):
        assert t.is_contiguous() and t.data_ptr() % 256 == 0
        assert bool((t.view(-1).view(torch.uint8) == fill).all())
    assert ws.dtype == torch.uint8 and ws.numel() == 1000
    if fill == 0xFF:
        assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and bool(torch.isnan(h).all()) and bool((d == -1).all())
    if fill == 0x7F:
        assert bool(torch.isfinite(a).all()) and float(a[0, 0, 0]) > 3e38 and float(b[0]) > 1e306 and int(d[0, 0]) > 2 ** 30
    if fill == 0x3C:
        assert 0.01 < float(a[0, 0, 0]) < 0.02 and 0 < float(b[0]) < 1e-15 and 1.0 < float(h[0, 0]) < 1.1
    assert H.check_guards() == []


def test_a_write_past_the_payload_is_reported_with_its_site(monkeypatch):
    with H.controlled_memory(monkeypatch, 0x7F):
        t = torch.empty((2, 5), dtype=torch.float32); line = _line()
    assert H.check_guards() == []
    flat = t.view(-1)
    torch.as_strided(flat, (11,), (1,))[10] = 1.0           # one element past the end: the first bytes of the back guard
    found = H.check_guards()
    assert len(found) == 1, found
    f = found[0]
    assert f["side"] == "back" and f["first"] in (0, 2, 3) and 1 <= f["count"] <= 4 and f["kind"] == "empty"
    assert f["site"] == f"tests/test_mem_table.py:{line}", f
    torch.as_strided(flat, (11,), (1,))[10] = float(torch.tensor([0x7F7F7F7F], dtype=torch.int32).view(torch.float32))
    assert H.check_guards() == []
    torch.as_strided(flat, (12,), (1,), storage_offset=flat.storage_offset() - 1)[0] = 0.0      # one element in front
    found = H.check_guards()
    assert len(found) == 1 and found[0]["side"] == "front" and found[0]["first"] == 0, found


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_a_write_into_a_guarded_input_is_reported():
    src = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    g = H.guarded(src); line = _line()
    tr = H.guarded(src.t())                                  # a dense permutation keeps its strides
    assert torch.equal(g, src) and g.data_ptr() % 256 == 0 and g.data_ptr() != src.data_ptr()
    assert tr.stride() == src.t().stride() and torch.equal(tr, src.t())
    assert H.check_inputs_untouched() == [] and H.check_guards() == []
    g[1, 2] = -0.0 if float(g[1, 2]) == 0.0 else -float(g[1, 2])
    bad = H.check_inputs_untouched()
    assert len(bad) == 1 and bad[0]["site"] == f"tests/test_mem_table.py:{line}" and bad[0]["changed"] == 1, bad
    # NaN payloads compare bitwise
    n = H.guarded(torch.full((4,), float("nan")))
    assert [b["site"] for b in H.check_inputs_untouched()] == [bad[0]["site"]]
    assert n.shape == (4,)


def test_an_element_aligned_copy():
    src = torch.randn(5, 4, dtype=torch.float32)
    g = H.guarded(src, offset_elems=1)
    assert torch.equal(g, src) and g.is_contiguous() and g.data_ptr() % 16 == 4
    # ... and what the package makes of it: a copy at a 16-byte address, the tensor itself when it already is aligned
    a = _lib.norm(g, torch.float32)
    assert a.data_ptr() % 16 == 0 and a.data_ptr() != g.data_ptr() and torch.equal(a, g)
    assert _lib.c(g).data_ptr() % 16 == 0 and torch.equal(_lib.c(g), g)
    al = H.guarded(src)
    assert _lib.norm(al, torch.float32) is al and _lib.c(al).data_ptr() == al.data_ptr()
    assert _lib.norm(g, torch.float64).dtype == torch.float64 and _lib.norm(None, torch.float32) is None
    assert H.check_inputs_untouched() == []


def test_workspace_keeps_key_growth_and_use_counts(monkeypatch):
    key = (None, 0, "bwd")
    before = _lib.workspace_uses(CPU, "bwd", 0)
    with H.controlled_memory(monkeypatch, 0x00) as st:
        a = _lib.workspace(CPU, 100, "bwd", stream=0)
        a[:10] = 7
        b = _lib.workspace(CPU, 50, "bwd", stream=0)         # smaller: the same buffer, content kept
        assert b.data_ptr() == a.data_ptr() and b.numel() == 100 and int(b[3]) == 7
        assert _lib.workspace_uses(CPU, "bwd", 0) == before + 2
        _lib.workspace_touch(CPU, "bwd", 0)
        assert _lib.workspace_uses(CPU, "bwd", 0) == before + 3
        c = _lib.workspace(CPU, 200, "bwd", stream=0)        # larger: a new one, clean
        assert c.numel() == 200 and not bool(c.any()) and _lib._ws_cache[key] is c
        other = _lib.workspace(CPU, 10, "fwd", stream=0)
        assert other.data_ptr() != c.data_ptr()
        assert (st["ws_created"], st["ws_reused"]) == (3, 1) and st["tags_created"] == {"bwd", "fwd"} and not st["tags_stale"]
        c[:] = 5
    # stale: the cached buffers keep what they hold, torch allocations are filled with torch_fill, a grown workspace too
    with H.controlled_memory(monkeypatch, None, torch_fill=0xFF) as st:
        d = _lib.workspace(CPU, 150, "bwd", stream=0)
        assert d.data_ptr() == c.data_ptr() and bool((d == 5).all())
        assert bool(torch.isnan(torch.empty(3)).all())
        e = _lib.workspace(CPU, 300, "bwd", stream=0)          # it has to grow: the old content at the head, torch_fill behind
        assert bool((e[:200] == 5).all()) and bool((e[200:] == 0xFF).all())
        assert (st["ws_created"], st["ws_reused"], st["ws_grown"]) == (0, 1, 1)
        n = _lib.workspace(CPU, 30, "lu", stream=0)            # a tag nobody used before: not stale
        assert bool((n == 0xFF).all()) and st["tags_stale"] == {"bwd"} and st["tags_created"] == {"lu"}
    assert H.check_guards() == []
    e.as_strided((301,), (1,))[300] = 1                      # a workspace's guards are checked too
    found = H.check_guards()
    assert len(found) == 1 and found[0]["kind"] == "workspace:bwd" and found[0]["side"] == "back" and found[0]["first"] == 0
    # a fresh context releases the cached workspaces
    with H.controlled_memory(monkeypatch, 0x3C):
        assert key not in _lib._ws_cache
        f = _lib.workspace(CPU, 20, "bwd", stream=0)
        assert bool((f == 0x3C).all())
    assert _lib.workspace.__module__ == "lqp_py_amd._lib"


def test_same_bits():
    nan = torch.tensor([float("nan"), 1.0])
    assert H.same_bits(nan, nan.clone()) and not H.same_bits(nan, torch.tensor([float("nan"), 2.0]))
    assert not H.same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and H.same_bits(None, None) and not H.same_bits(None, nan)
    assert H.same_bits(3, 3) and not H.same_bits(3, 4) and not H.same_bits(nan, nan.double())


# ---------------------------------------------------------------------------------------------------------------------------------
# every allocation site of the package is one the harness intercepts
def test_every_allocation_site_is_intercepted():
    sites = MT.allocation_sites()
    assert len(sites) >= 40, len(sites)
    missed = [f"{f}:{ln} {text}" for f, ln, prefix, what, text in sites
              if not MT.intercepted(prefix, what) and f"{f}:{ln} {text}" not in MT.NOT_INTERCEPTED]
    assert not missed, missed
    assert MT.aliases() == [], "torch.empty / _lib.workspace bound to another name escapes tests/memharness.py"
    stale = [k for k in MT.NOT_INTERCEPTED if k not in {f"{f}:{ln} {text}" for f, ln, _p, _w, text in sites}]
    assert not stale, stale


def test_the_scan_sees_what_it_must():
    assert MT.intercepted("torch.", "empty") and MT.intercepted("_lib.", "workspace") and MT.intercepted("torch.", "empty_like")
    assert not MT.intercepted("", "empty") and not MT.intercepted("x.", "new_empty") and not MT.intercepted("th.", "empty")
    found = {(p, w) for p, w in ((m.group(1), m.group(2)) for m in MT.ALLOC_RE.finditer(
        "a = empty((3,)); b = x.new_empty(3); c = torch.empty_like(t); d = _lib.workspace(dev, 3, 'fwd'); e = th.empty(1)"))}
    assert found == {("", "empty"), ("x.", "new_empty"), ("torch.", "empty_like"), ("_lib.", "workspace"), ("th.", "empty")}


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage
def _rows(table):
    return [r["row"] for r in MT.ROWS if r["table"] == table]


def test_rows_exist_and_every_before_meets_its_rule():
    for r in MT.ROWS:
        assert r["table"] in MT.TABLES and r["row"] in MT.TABLE_ROWS[r["table"]], r
        assert MT.before_ok(r) == [], (r["id"], MT.before_ok(r))
    for t, n in MT.MISALIGNED:
        assert n in MT.TABLE_ROWS[t] and MT.home(t, n)["n"] % 4 == 0, (t, n)
    what = [MT.home(t, n)["sig"]["linsolve_used"] if t == "tier" else MT.home(t, n)["form"] for t, n in MT.MISALIGNED]
    assert what == [2, 1, "chol"]          # the sweep tier, the LU tier, the Cholesky backward


def test_every_before_leaves_a_workspace_the_row_fits_in():
    """(the library's host-side *_workspace_bytes queries: no GPU needed)"""
    for r in MT.ROWS:
        small = MT.before_bytes_ok(r)
        assert bool(small) == (r["id"] in MT.GROWS), (r["id"], small, MT.workspace_bytes(r["table"], r["row"]), MT.workspace_bytes(*r["before"]))
    assert set(MT.GROWS) <= set(MT.ROW_BY_ID)


def test_the_before_rule_can_fail():
    same = MT.row("tier", "small_n65_m0", "small_n1_m0")             # smaller in B and n, same m, same tier, same dtype
    assert len(MT.before_ok(same)) == 2
    assert MT.before_ok(MT.row("fp", "chol_nf1_n130", ("direct", "solve_n257_f64")))[0][0] == "no workspace tag in common"
    assert MT.before_ok(MT.row("fp", "chol_nf1_n130", "nonsense"))[0][0] == "no such row"


def test_required_rows():
    for table, names in MT.REQUIRED.items():
        assert set(names) <= set(_rows(table)), (table, set(names) - set(_rows(table)))
    # every loop kind and factorisation family of plan_forward, by what the rows' signatures and names say
    sigs = [MT.home("tier", n) for n in _rows("tier")]
    assert {r["sig"]["linsolve_used"] for r in sigs} == {1, 2} and {r["dtype"] for r in sigs} == {"f32", "f64"}
    assert {r["sig"].get("loop_workgroups") for r in sigs if r["sig"]["linsolve_used"] == 2} >= {1, 2, 4}
    assert {r["sig"]["mode_used"] for r in sigs} == {1, 2} and any(r["n"] > 1024 for r in sigs) and any(r["K"] > 60 for r in sigs)


def test_fixed_point_backward_rows():
    rows = [FT.ROW_BY_NAME[n] for n in _rows("fp")]
    assert {r["entry"] for r in rows} == set(FT.ENTRIES)
    nfs = set().union(*(FT.nf_values(r) for r in rows))
    assert 0 in nfs and 1 in nfs and any(v % 64 == 1 and v > 1 for v in nfs)
    assert any(isinstance(r["nf"], list) and len({-(-v // 64) for v in r["nf"]}) > 2 for r in rows)      # mixed block counts
    assert any(r["form"] == "fallback" for r in rows) and any(r["want"] for r in rows)
    kkt = [KT.ROW_BY_NAME[n] for n in _rows("kkt")]
    assert len(kkt) >= 2 and any(r["sides"] in ("lb", "ub") for r in kkt) and any(r["sides"] == "both" for r in kkt)


def test_unroll_direct_and_each_rows():
    un = [U.ROW_BY_NAME[n] for n in _rows("unroll")]
    assert {r["env"].get("LQP_UNROLL_NATIVE", "1") for r in un} == {"0", "1"}
    assert any(r["family"] in ("ev32", "ev64") for r in un)
    di = [MT.home("direct", n) for n in _rows("direct")]
    assert any(r["family"] == "solve" and r["N"] % 4 != 0 and r["N"] % 64 == 1 for r in di)
    assert {"solve", "lulayer", "eqcon", "optnet", "layer0"} <= {r["family"] for r in di}
    assert set(_rows("each")) <= set(MT.EACH_CALL) and all(MT.ROW_BY_ID[f"each:{n}"]["before"][1] in MT.EACH_CALL for n in _rows("each"))


def test_every_workspace_tag_is_exercised():
    found, calls = MT.workspace_tags_in_sources()
    assert calls >= 6 and found == {"fwd", "bwd", "lu", "kkt", "unroll"}, (found, calls)
    used = set().union(*(MT.tags(r["table"], r["row"]) for r in MT.ROWS))
    assert found <= used, found - used


def test_modes_and_sizes():
    assert MT.MODES == ("fresh-00", "fresh-FF", "fresh-7F", "fresh-3C", "stale")
    assert {m.split("-")[1] for m in MT.MODES if m != "stale"} == set(H.FILLS)
    # no row larger than its table's: they ARE the tables' rows
    assert all(r["row"] in MT.TABLE_ROWS[r["table"]] and r["before"][1] in MT.TABLE_ROWS[r["before"][0]] for r in MT.ROWS)
    assert os.path.exists(os.path.join(os.path.dirname(MT.PACKAGE), "docs", "WORKSPACE.md"))
