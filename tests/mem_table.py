"""What the memory tests run, as data (no GPU needed to import this module): tests/test_gpu_mem.py runs every row under every mode of
tests/memharness.py, tests/test_mem_table.py checks the coverage rules below without a GPU.  docs/WORKSPACE.md is the audit the rows
stand on: which region of which buffer is written first by whom.

A row names a row of one of the existing tables -- shapes, inputs, controls, environment overrides, bars and oracles are that row's
and are not restated:
  table    "tier" (tier_table) | "fp" (fp_table) | "kkt" (kkt_table) | "unroll" (unroll_table) | "direct" (direct_table) | "each" (each_table)
  row      its name there
  before   (table, row): the call that precedes it in the mode `stale`, on the same cached workspaces.  It is larger in at least one
           of B, n, m (what it leaves behind reaches past the new layout's regions), differs in tier or dtype (the offsets of the
           layout move) and uses a workspace tag the row uses.  Its buffer of every shared tag is at least as large as the row's
           (workspace_bytes), so that the row really runs in what it left -- GROWS lists the exceptions.

Modes: fresh-00 | fresh-FF | fresh-7F | fresh-3C (every buffer filled with that byte, memharness.FILLS) and stale.
"""
import os
import re

import direct_table as DT
import each_table as ET
import fp_table as FT
import kkt_table as KT
import tier_table as T
import unroll_table as U

MODES = ("fresh-00", "fresh-FF", "fresh-7F", "fresh-3C", "stale")
TABLES = ("tier", "fp", "kkt", "unroll", "direct", "each")
NOMINAL_CUS = 256          # batch sizes written as expressions of the CU count are compared at this one


def row(table, name, before):
    if isinstance(before, str):
        before = (table, before)
    return dict(table=table, row=name, before=tuple(before), id=f"{table}:{name}")


# the forward rows run the functional solve and the module's forward + backward (test_gpu_tiers._run): tags "fwd" and "bwd"
_F64_LU = "lu2_n450_f64"           # n = 450, m = 3, B = 4, float64, the one-workgroup-per-matrix LU with launch_mode 1
ROWS = [
    # ---------------- every LoopKind and factorisation family of plan_forward ----------------
    row("tier", "small_n65_m0", _F64_LU),
    row("tier", "small_n31_m1", _F64_LU),
    row("tier", "sweep2_n129_m1", _F64_LU),
    row("tier", "sweep2_n257_m16", "big_n513_m2"),
    row("tier", "sweep4_n449_m16", "turns_n449_half1"),
    row("tier", "turns_n449_half1", "big_many_n600"),
    row("tier", "sweep1_n330_turns0", "turns_n449_half1"),
    row("tier", "sweepml_n330_m2", _F64_LU),
    row("tier", "loop_split0_n330", _F64_LU),
    row("tier", "mode1_n330", _F64_LU),
    row("tier", "mode2_nosync_n330", _F64_LU),
    row("tier", "events_lo_n330", _F64_LU),
    row("tier", "events_hi_n449_mode1", "big_n513_m2"),
    row("tier", "big_n513_m2", "wide_n1025_f32"),
    row("tier", "big_many_n600", "turns_n330_cus3"),
    row("tier", "lu_m17_n200", _F64_LU),
    row("tier", "lu_nonsym_n200_f64", "lu2_n450_f32"),
    row("tier", "lu1_n300_f64", "lu2_n450_f32"),
    row("tier", "lu2_n450_f32", "big_n1000_m1"),
    row("tier", "dense_n200_f32", _F64_LU),
    row("tier", "dense_n256_f64", "lu2_n450_f32"),
    row("tier", "densew_n257_f64", "lu2_n450_f32"),
    row("tier", "wide_n1025_f32", "bigl_n1100_f64"),
    # ---------------- stop='each': the per-problem words behind everything else, the ring refilled by the host ----------------
    row("each", "small_n50_event", "f64_n70_m3_event"),
    row("each", "split_n130_event", "split_n449"),
    row("each", "chunk_n20", "f64_n70_m3"),
    row("each", "f64_n70_m3", "split_n130"),
    # ---------------- the fixed-point backward: every entry, free sets of 0, 1 and 64 k + 1, mixed block counts, the fall-back ----
    row("fp", "chol_nf0_m1_n130", "lu_nf257_n300_f64"),
    row("fp", "chol_nf1_n130", "lu_nf257_n300_f64"),
    row("fp", "chol_nf64_n150", "lu_nf257_n300_f64"),             # want=True
    row("fp", "chol_nf65_n150", "lu_nf257_n300_f64"),
    row("fp", "chol_mixed_n576", "planner_n1025_m0"),
    row("fp", "fallback_indef_n200", "lu_nf257_n300_f64"),
    row("fp", "chol_pre_nf65_n150", "lu_nf257_n300_f64"),         # want=True
    row("fp", "lu_nf65_n150_f64", "chol_m3_nf200_n330"),
    row("fp", "lu_pre_n150_f64", "chol_m3_nf200_n330"),
    # ---------------- backward='kkt' ----------------
    row("kkt", "chol_n65_m3", "lu_n150_f64"),
    row("kkt", "chol_ub_n130", "lu_n150_f64"),
    # ---------------- unroll=True: LQP_UNROLL_NATIVE at both values, the LU tape, a tape through a rho event ----------------
    row("unroll", "split_n257_m1", "lu64_n450_m3"),
    row("unroll", "lu64_n60_m1", "split_n320_m2"),
    row("unroll", "native0_n200_m1", ("direct", "solve_n257_f64")),
    row("unroll", "ev32_grow_n330", ("direct", "solve_n513_f64")),
    # ---------------- the entry points without a loop ----------------
    row("direct", "solve_n65_k3_f32", "solve_n129_f64"),          # N % 4 == 1, N % 64 == 1
    row("direct", "solve_n129_f64", "solve_n513_f32"),
    row("direct", "lulayer_n65_k3_f32", "solve_n129_f64"),
    row("direct", "eqcon_n60_m5_f32", "eqcon_n100_m17_f64"),      # N = 65
    row("direct", "eqcon_n100_m17_f64", "eqcon_n130_m65_f32"),
    row("direct", "optnet_n130_m3_f32", "eqcon_n130_m65_f32"),
    row("direct", "layer0_dense2_n128_m1_f32", "layer0_densew_n257_m2_f64"),
    row("direct", "layer0_densew_n257_m2_f64", "layer0_loop1_n600_m2_f32"),
]
ROW_BY_ID = {r["id"]: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS), "duplicate rows"

# inputs at an address that is only element-aligned (flat[1:1 + numel].view(shape)): the sweep tier, the LU tier, the Cholesky backward,
# each at n % 4 == 0, where the kernels take 16-byte loads
MISALIGNED = [("tier", "sweep2_n256_m0"), ("tier", "lu_m17_n200"), ("fp", "chol_nf128_n200")]

# the least the rows must hold, by name (tests/test_mem_table.py; the rules by property are there too)
REQUIRED = {
    "tier": ("small_n65_m0", "small_n31_m1", "sweep2_n129_m1", "sweep2_n257_m16", "sweep4_n449_m16", "turns_n449_half1",
             "sweep1_n330_turns0", "sweepml_n330_m2", "loop_split0_n330", "mode1_n330", "mode2_nosync_n330", "events_lo_n330",
             "events_hi_n449_mode1", "big_n513_m2", "big_many_n600", "lu_m17_n200", "lu_nonsym_n200_f64", "lu1_n300_f64", "lu2_n450_f32",
             "dense_n200_f32", "dense_n256_f64", "densew_n257_f64", "wide_n1025_f32"),
    "each": ("small_n50_event", "split_n130_event", "chunk_n20", "f64_n70_m3"),
    "fp": ("chol_mixed_n576",),
}

# how a row of tests/each_table.py is called: (extra control keys, environment, SB._SYNC_SPLIT or None, the problems compared with
# their solo oracle (None: all), kind of loop) -- the case of tests/test_gpu_each.py the row is named for
EACH_CALL = {
    "small_n50_event": ({}, {}, None, None, "small"),
    "split_n130_event": ({}, {}, None, None, "split2"),
    "split_n130": ({}, {}, None, None, "split2"),
    "split_n449": ({}, {}, None, None, "split4"),
    "f64_n70_m3": ({}, {}, None, None, "one_f64"),
    "f64_n70_m3_event": ({}, {}, None, None, "one_f64"),
    "chunk_n20": ({}, {"LQP_SYNC_PLAN": "0"}, False, "done", "small_chunked"),      # test_host_driven_persistent_chunks
}

TABLE_ROWS = {"tier": T.ROW_BY_NAME, "fp": FT.ROW_BY_NAME, "kkt": KT.ROW_BY_NAME, "unroll": U.ROW_BY_NAME, "direct": DT.ROW_BY_NAME,
              "each": ET.ROWS}


def home(table, name):
    return TABLE_ROWS[table][name]


def dims(table, name, cus=NOMINAL_CUS):
    """(B, n, m, dtype "f32" | "f64") of a row"""
    r = home(table, name)
    if table == "each":
        import torch
        return r["B"], r["n"], r["m"], "f64" if r["dtype"] == torch.float64 else "f32"
    return T.batch(r, cus), r["n"], r["m"], r["dtype"]


def tags(table, name):
    """The workspace tags (_lib.workspace) the row's call asks for"""
    r = home(table, name)
    if table == "tier":
        return {"fwd", "bwd"}
    if table == "each":
        return {"fwd"}
    if table == "fp":
        return {"bwd"}
    if table == "kkt":
        return {"kkt"} if r["entry"] == "composed" else {"bwd"}
    if table == "unroll":
        # the solve of an unroll forward runs on a private buffer; the native sweep takes its tape from "unroll", the walk through rho
        # events and the taped loop of torch ops factorise with lu_layer.lu_factor
        return {"lu"} if r["family"] in ("taped", "ev32", "ev64") else {"unroll"}
    fam = r["family"]
    if fam in ("solve", "lulayer"):
        return {"lu"} if r["factor"] == "hip" else set()
    if fam in ("eqcon", "uncon", "optnet"):
        return {"kkt"}
    return {"fwd", "bwd"}


def tier_key(table, name):
    """What the row's call runs, as far as the tables say it: two rows with different keys lay out or use their workspace differently"""
    r = home(table, name)
    if table == "tier":
        return ("tier", tuple(sorted(r["sig"].items())), tuple(sorted(r["env"].items())), tuple(sorted(r["ctl"].items())))
    if table == "each":
        return ("each", EACH_CALL[name][4])
    if table in ("fp", "kkt"):
        return (table, r["form"], T.ks(max(FT.nf_values(r))) if table == "fp" else T.ks(r["n"]))
    if table == "unroll":
        return ("unroll", r["family"])
    return ("direct", r["family"], r["tier"], T.ks(r["N"]))


def before_ok(r):
    """-> the list of rules the row's `before` breaks (empty: fine)"""
    bad = []
    (bt, bn), (t, n) = r["before"], (r["table"], r["row"])
    if bn not in TABLE_ROWS[bt]:
        return [("no such row", bt, bn)]
    Bb, nb, mb, db = dims(bt, bn)
    B, nn, m, d = dims(t, n)
    if not (Bb > B or nb > nn or mb > m):
        bad.append(("not larger in B, n or m", (Bb, nb, mb), (B, nn, m)))
    if not (db != d or tier_key(bt, bn) != tier_key(t, n)):
        bad.append(("same tier and dtype",))
    if tags(t, n) and not (tags(bt, bn) & tags(t, n)):
        bad.append(("no workspace tag in common", sorted(tags(bt, bn)), sorted(tags(t, n))))
    return bad


def workspace_bytes(table, name, cus=NOMINAL_CUS):
    """{tag: bytes the row's call asks _lib.workspace for}, from the library's own *_workspace_bytes queries (host functions)"""
    from lqp_py_amd import _lib
    lib = _lib.load()
    B, n, m, d = dims(table, name, cus)
    dt = _lib.LQP_F32 if d == "f32" else _lib.LQP_F64
    r = home(table, name)
    out = {}
    for tag in tags(table, name):
        if tag == "fwd":
            out[tag] = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m)
        elif tag == "bwd":
            out[tag] = lib.lqp_boxqp_backward_fp_workspace_bytes(dt, B, n, m)
        elif tag == "lu":
            out[tag] = lib.lqp_lu_factor_workspace_bytes(dt, B, n + m)
        elif tag == "kkt":
            out[tag] = lib.lqp_kkt_solve_workspace_bytes(dt, B, n, m)
        else:
            assert tag == "unroll"
            out[tag] = (lib.lqp_boxqp_unroll_backward_lu_workspace_bytes(dt, B, n, m, r["K"]) if r["family"] in ("lu32", "lu64") else
                        lib.lqp_boxqp_unroll_backward_workspace_bytes(B, n, m, r["K"]))
    return out


# rows whose `before` leaves a SMALLER buffer of a shared tag: the buffer grows in the stale run, and the harness carries the old
# content over to the head of the new one (memharness._make_workspace) -- each with its reason
GROWS = {
    "tier:big_many_n600": "the largest workspace of the tables (129 problems of 600 rows): its `before` is the largest batch, "
                          "turns_n330_cus3, whose per-problem regions at the front of the layout reach further",
}


def before_bytes_ok(r):
    """-> the shared tags for which the `before` call leaves a smaller buffer than the row asks for"""
    a, b = workspace_bytes(r["table"], r["row"]), workspace_bytes(*r["before"])
    return sorted(t for t in a if t in b and b[t] < a[t])


# ---------------------------------------------------------------------------------------------------------------------------------
# source scans (tests/test_mem_table.py)
PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lqp_py_amd")
ALLOC_RE = re.compile(r"(?<![\w.])((?:[\w.]+\.)?)(empty|empty_like|new_empty|workspace)\(")
# allocation sites the harness does not intercept, each with its reason: "file.py:line text" -> reason (none)
NOT_INTERCEPTED = {}


def package_sources():
    return sorted(os.path.join(PACKAGE, f) for f in os.listdir(PACKAGE) if f.endswith(".py"))


def allocation_sites():
    """-> [(file, line number, prefix, what, text)] of every `empty(`, `empty_like(`, `new_empty(` and `workspace(` call in lqp_py_amd/*.py
    (definitions -- `def workspace(` -- left out)"""
    out = []
    for path in package_sources():
        with open(path) as fh:
            for i, line in enumerate(fh, 1):
                code = line.split("#", 1)[0]
                if re.match(r"\s*def\s", code):
                    continue
                for mt in ALLOC_RE.finditer(code):
                    out.append((os.path.basename(path), i, mt.group(1), mt.group(2), line.strip()))
    return out


def intercepted(prefix, what):
    """Is a call written `prefix what(` one the harness replaces?  torch.empty( / torch.empty_like( / _lib.workspace( are attribute
    look-ups at the call; inside _lib.py `workspace` is not called and `torch.empty(` is the same look-up."""
    return (what in ("empty", "empty_like") and prefix == "torch.") or (what == "workspace" and prefix == "_lib.")


def aliases():
    """-> lines of lqp_py_amd/*.py that bind torch.empty / torch.empty_like / _lib.workspace to another name (a default argument, an
    assignment, a from-import): such a name would escape the harness"""
    pat = re.compile(r"(from\s+torch\s+import\b.*\bempty)|(=\s*torch\.empty(_like)?\b(?!\())|(=\s*_lib\.workspace\b(?!\())|"
                     r"(from\s+\._lib\s+import\b.*\bworkspace\b)|(\bworkspace\s+as\b)")
    out = []
    for path in package_sources():
        with open(path) as fh:
            for i, line in enumerate(fh, 1):
                code = line.split("#", 1)[0]
                if pat.search(code):
                    out.append(f"{os.path.basename(path)}:{i} {line.strip()}")
    return out


def workspace_tags_in_sources():
    """-> the set of tags passed to _lib.workspace anywhere in lqp_py_amd/*.py (every call passes a string literal)"""
    found, calls = set(), 0
    for path in package_sources():
        with open(path) as fh:
            src = fh.read()
        for mt in re.finditer(r"_lib\.workspace\(", src):
            calls += 1
            depth, j = 1, mt.end()
            while depth and j < len(src):
                depth += {"(": 1, ")": -1}.get(src[j], 0)
                j += 1
            lit = re.findall(r"""["'](\w+)["']""", src[mt.end():j])
            assert len(lit) == 1, (path, src[mt.start():j])
            found.add(lit[0])
    return found, calls
