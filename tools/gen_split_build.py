#!/usr/bin/env python3
"""Split build of the HIP library: one translation unit per group of kernels, compiled in parallel.

Every kernel is a template, so the host code (csrc/lqp_amd.hip) is compiled with `extern template` declarations of every
instance (no device code of theirs at all) while each group's translation unit instantiates its share explicitly -- same
headers, same flags, the same code per kernel as the single-source build (LQP_UNITY_BUILD=1).

KERNELS below is the manifest: every kernel instance the library contains.  An instance the host code names that is missing
here would be compiled into the host translation unit silently; tests/test_abi_and_host.py fails on that.

    python tools/gen_split_build.py            # (re)writes csrc/split/*.inc / *.hip
    python tools/gen_split_build.py --out DIR  # ... somewhere else
    python tools/gen_split_build.py --check    # writes nothing; exit status 1 when csrc/split/ is not what it would write
"""
import argparse
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "lqp_py_amd", "csrc", "split")



def loop(kernel, form, args=""):
    """predicate: an instance of a loop kernel (the form tag is its last template argument) whose other arguments begin with `args`"""
    return lambda n: re.search(rf"{kernel}<{args}[^>]*lqp::Form{form}>", n)


def term_groups(g, tag):
    """the groups of the instances with a separable term's step (lqp::Form<tag>, lqp::Term<tag>), grouped as their plain twins are"""
    own = rf"k_(fwd_epilogue|term_setup)<\w+, lqp::Term{tag}>|k_{g}_"
    return [
        (f"split_{g}_c", loop("k_admm_loop_split", tag, r"(3|4), 512, false, 2,")),
        (f"split_{g}_a", loop("k_admm_loop_split", tag, r"(5|6|7), 512, false, 2,")),
        (f"split_{g}_b", loop("k_admm_loop_split", tag)),
        (f"loop_{g}_tail", loop("k_admm_loop", tag, r"\w+, \w+, true,")),
        (f"loop_{g}_hot", loop("k_admm_loop", tag)),
        (g, lambda n: loop("k_admm_loop_np2", tag)(n) or loop("k_admm_loop_small", tag)(n) or re.search(own, n)),
    ]


# the separable terms (lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber): (group suffix, tag of lqp::Form* and lqp::Term*).  A new term is one entry here
# and its backward's element-wise kernels in KERNELS.
TERMS = [("l1", "L1"), ("soft", "Soft"), ("log", "Log"), ("pwl", "Pwl"), ("huber", "Huber")]
# group -> predicate on the demangled name; first match wins.  Balanced by measured compile time (seconds at -O3).
GROUPS = [grp for g, tag in TERMS for grp in term_groups(g, tag)] + [
    ("bwd_f", lambda n: re.search(r"k_bwd_chol_solve<\d, true>", n)),
    ("resident_f", lambda n: re.search(r"k_spd_resident<8, 2, true>", n)),
    ("resident_g", lambda n: re.search(r"k_spd_resident<(5|6|7), 2, true>", n)),
    ("resident_h", lambda n: re.search(r"k_spd_resident<\d, \d, true>", n)),
    ("resident_c", lambda n: re.search(r"k_spd_resident<(3|4), 2(, false)?>", n)),
    ("resident_a", lambda n: re.search(r"k_spd_resident<(5|6|7), 2(, false)?>", n)),
    ("resident_b", lambda n: re.search(r"k_spd_resident<8, 2(, false)?>|k_spd_resident<\d, 4(, false)?>", n)),
    ("split_c", loop("k_admm_loop_split", "All", r"(3|4), 512, false, 2,")),
    ("split_a", loop("k_admm_loop_split", "All", r"(5|6|7), 512, false, 2,")),
    ("split_b", loop("k_admm_loop_split", "All")),
    ("split_each_b", loop("k_admm_loop_split", "Each", r"((3|4|8), 512, false, 2|\d, 512, false, 4),")),
    ("split_each_a", loop("k_admm_loop_split", "Each")),
    ("loop_each_certify_tail", loop("k_admm_loop", "Certify", r"\w+, \w+, true,")),
    ("loop_each_certify_hot", loop("k_admm_loop", "Certify")),
    ("loop_each_detect_tail", loop("k_admm_loop", "Detect", r"\w+, \w+, true,")),
    ("loop_each_detect_hot", loop("k_admm_loop", "Detect")),
    ("loop_each_tail", loop("k_admm_loop", "Each", r"\w+, \w+, true,")),
    ("loop_each_hot", loop("k_admm_loop", "Each")),
    ("loop_tail", loop("k_admm_loop", "All", r"\w+, \w+, true,")),
    ("loop_hot", loop("k_admm_loop", "All")),
    ("dense", lambda n: "k_lu_inverse<" in n or "k_admm_loop_dense" in n),
    ("lu2", lambda n: "k_lu_factor2<" in n),
    ("lu_a", lambda n: re.search(r"k_lu_factor<float, (32|16), true|k_lu_factor_big|k_lu_factor_wide", n)),
    ("lu_b", lambda n: "k_lu_factor<" in n),
    ("spd", lambda n: re.search(r"k_spd_|k_bwd_chol_solve|k_bwd_build_chol|k_debug_chol_solve|k_debug_chol_factor", n)),
    ("unroll", lambda n: "k_unroll_" in n or loop("k_admm_loop_small", "All")(n)),
    ("misc", lambda n: True),
]

# ---- the manifest: (kernel, parameter signature, template-argument tuples).  {0} in a signature is the first template argument ----
BOTH, F32, ZERO = [("double",), ("float",)], [("float",)], [(0,)]
FP, BP, ULP = "lqp::FwdParams<{0}>", "lqp::BwdParams<{0}>", "lqp::UnrollLuParams<{0}>"
FPF, BPF = "lqp::FwdParams<float>", "lqp::BwdParams<float>"
KS_NP = [(3, 2), (4, 2), (5, 2), (6, 2), (7, 2), (8, 2), (7, 4), (8, 4)]      # Ks, workgroups per problem (four: Ks = 7, 8 only)
# The forms of the loop kernels (the tags of lqp_boxqp.hpp), the last template argument of every instance: the batch stops as one |
# control['stop'] = 'each' | ... with the infeasibility certificate (control['infeasible']) | ... and the dual certificate beside it
# (control['unbounded']) | one per separable term (TERMS): that term's step
ALL, EACH, DETECT, CERTIFY = ("lqp::Form" + f for f in ("All", "Each", "Detect", "Certify"))
TERM_FORMS = tuple("lqp::Form" + tag for _, tag in TERMS)
TERM_TAGS = tuple("lqp::Term" + tag for _, tag in TERMS)
FORMS = (ALL, EACH, DETECT, CERTIFY) + TERM_FORMS
SPLIT = [(ks, 512, False, np_) for ks, np_ in KS_NP]
# the one-workgroup loop, hot and continuation: LU f64 | LU f32 | LU f32 resident | symmetric
LOOP = [(t, res, tail, 1024, sym) for tail in (False, True)
        for t, res, sym in (("double", False, False), ("float", False, False), ("float", True, False), ("float", True, True))]
in_forms = lambda args, forms: [a + (f,) for f in forms for a in args]
LOOP_SIG = FP + ", int, int, int, int, int"
LU_SIG = "{0}*, int, int, unsigned long, int*, int, int*, int const*"
WIDE_SIG = LU_SIG + ", int const*, int*, unsigned long, unsigned int, int, unsigned long long*"
KERNELS = [
    # the ADMM loops (lqp_boxqp.hpp, lqp_loop_split.hpp, lqp_loop_small.hpp, lqp_dense.hpp)
    ("k_admm_loop", LOOP_SIG, in_forms(LOOP, FORMS) + [("float", True, False, 512, False, ALL), ("float", True, False, 512, True, ALL)]),
    ("k_admm_loop_split", FPF + ", int, int, int", in_forms(SPLIT, (ALL, EACH) + TERM_FORMS) + [(8, 512, True, 2, ALL)]),      # (EACH serves DETECT and CERTIFY)
    ("k_admm_loop_small", FPF + ", int, int, int", in_forms([()], FORMS)),
    ("k_admm_loop_np2", FPF + ", int, int, int, int, int", in_forms([()], (ALL,) + TERM_FORMS)),
    ("k_admm_loop_dense", FP + ", int, int, int", BOTH),
    ("k_admm_loop_dense_w", FP + ", int, int, int, int", BOTH),
    # the symmetric x-update (lqp_spd.hpp)
    ("k_spd_resident", FPF + ", int const*", [(ks, np_, f16) for ks, np_ in KS_NP for f16 in (False, True)]),
    ("k_spd_prep", FPF, ZERO),
    ("k_spd_rho_big", FPF, ZERO),
    ("k_spd_begin", FPF + ", int const*", ZERO),
    ("k_spd_end", FPF + ", int const*", ZERO),
    ("k_spd_step", FPF + ", int const*, int, int", ZERO),
    ("k_spd_big_step", FPF + ", int const*, int, int", ZERO),
    ("k_spd_inverse", FPF + ", int const*", [(1,), (2,)]),
    ("k_spd_inverse_dense", "float const*, float*, float*, int*, int, int, float*", [(1,), (2,)]),
    ("k_debug_chol_factor", "float*, int const*, int*, int, int, int", [(False,), (True,)]),
    ("k_debug_chol_solve", "float const*, int const*, float const*, float*, int, int, int", [(2,), (4,)]),
    # the pivoted LU (lqp_lu.hpp: one workgroup, one or several panel rows per thread; lqp_lu2.hpp; lqp_lu_wide.hpp) and what runs on its factor
    ("k_lu_factor", LU_SIG + ", unsigned long long*, int const*",
     [("float", pb, mfma, nt) for mfma in (False, True) for pb, nt in ((16, 1024), (16, 512), (32, 512))] +
     [("float", 8, False, nt) for nt in (1024, 512)] + [("double", pb, True, nt) for pb in (8, 16) for nt in (1024, 512)]),
    ("k_lu_factor2", LU_SIG + ", int const*, unsigned long long*, unsigned long, unsigned int, unsigned long long*, int, int",
     [("double", 16), ("float", 32)]),
    ("k_lu_factor_big", LU_SIG + ", int const*", BOTH),
    ("k_lu_factor_wide", WIDE_SIG, BOTH),
    ("k_lu_factor_wide_tall", WIDE_SIG, F32),
    ("k_lu_inverse", "{0} const*, unsigned long, int, int, int const*, int, {0}*, unsigned long, int, int const*",
     [("double", False), ("float", False), ("float", True)]),
    ("k_pack", "{0} const*, int, int, unsigned long, int const*, int, {0}*, unsigned long, int*, int, int, int const*, int const*", BOTH),
    ("k_packed_solve", "{0} const*, int, int, int, int const*, {0}*, int, unsigned long, int, int, int const*", BOTH),
    # forward prologue / epilogue and the copies out of the workspace
    ("k_fwd_setup", FP, BOTH),
    ("k_fwd_epilogue", FP, BOTH),
    ("k_fwd_epilogue", FP + ", {0}*, {0}*", in_forms(BOTH, TERM_TAGS)),
    ("k_term_setup", FP + ", lqp::TermIn<{0}>", in_forms(BOTH, TERM_TAGS)),
    # ... and the element-wise kernels of the terms' backwards, whose sets differ
    ("k_l1_effective_box", "{0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0}, int, unsigned long, {0}*, {0}*, {0}*, {0}*", BOTH),
    ("k_l1_finish_grads", "{0} const*, {0} const*, {0} const*, {0} const*, unsigned long, {0}*, {0}*, {0}*, {0}*", BOTH),
    ("k_soft_effective_box", "{0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0}, int, unsigned long, {0}*, {0}*, {0}*, {0}*", BOTH),
    ("k_soft_finish_grads", "{0} const*, {0} const*, {0} const*, {0} const*, {0} const*, unsigned long, {0}*, {0}*, {0}*, {0}*, {0}*, {0}*", BOTH),
    ("k_log_effective_duals", "{0} const*, {0} const*, {0}, int, unsigned long, {0}*, {0}*", BOTH),
    ("k_log_finish_grads", "{0} const*, {0} const*, {0} const*, unsigned long, {0}*", BOTH),
    ("k_pwl_effective_box", "{0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0} const*, int, {0} const*, {0}, int, unsigned long, {0}*, {0}*, {0}*, {0}*", BOTH),
    ("k_pwl_finish_grads", "{0} const*, {0} const*, {0} const*, {0} const*, {0} const*, int, unsigned long, {0}*, {0}*, {0}*, {0}*", BOTH),
    ("k_huber_effective_duals", "{0} const*, {0} const*, {0} const*, {0} const*, {0}, int, unsigned long, {0}*, {0}*, {0}*", BOTH),
    ("k_huber_finish_grads", "{0} const*, {0} const*, {0} const*, {0} const*, {0} const*, {0} const*, unsigned long, {0}*, {0}*, {0}*", BOTH),
    ("k_rho_update", FP + ", int, int", BOTH),
    ("k_snap_init", "{0}*, unsigned long, int", BOTH),
    ("k_check_done", "int*, unsigned int const*, int, int", ZERO),
    ("k_report_info", "int const*, int*, int", ZERO),
    ("k_copy_ints", "int const*, int, int*, int, int", [("int",)]),
    ("k_copy_iters", "int const*, int*, int", ZERO),
    ("k_copy_pstatus", "int const*, int*, int", ZERO),
    ("k_copy_trace", "unsigned int const*, float*, int", ZERO),
    ("k_copy_matrix", "{0} const*, int, unsigned long, {0}*, int, unsigned long, int", BOTH),
    ("k_copy_residuals", "{0} const*, {0}*, {0}*, int", BOTH),
    # backward
    ("k_bwd_chol_solve", BPF, [(r, f16) for r in (0, 4) for f16 in (False, True)]),
    ("k_bwd_build_chol", BPF, ZERO),
    ("k_bwd_build", BP, BOTH),
    ("k_bwd_build_reduced", BP, BOTH),
    ("k_bwd_gather_rhs", BP, BOTH),
    ("k_bwd_residual", BP, BOTH),
    ("k_bwd_epilogue", BP, BOTH),
    ("k_kkt_build", "{0} const*, {0} const*, {0} const*, {0} const*, int, int, int, {0}*, {0}*, int*", BOTH),
    ("k_kkt_unpack", "{0} const*, int, int, int, {0}*, {0}*", BOTH),
    ("k_outer_grads", "{0} const*, {0} const*, {0} const*, {0} const*, int, int, {0}*, {0}*", BOTH),
    # unroll=True (lqp_unroll.hpp)
    ("k_unroll_sweep", FPF + ", lqp::UnrollParams", [(1,), (16,)]),
    ("k_unroll_sweep_split", FPF + ", lqp::UnrollParams, unsigned int", [(5, 16), (6, 16), (7, 16), (8, 16), (8, 1)]),
    ("k_unroll_sweep_lu", FP + ", " + ULP, BOTH),
    ("k_unroll_lu_eq", ULP + ", int, int", BOTH),
    ("k_unroll_outer", "float const*, float const*, float*, int, int", ZERO),
    ("k_unroll_outer_any", "{0} const*, {0} const*, {0}*, int, int", BOTH),
    ("k_unroll_scale_colmax", "float const*, int, float*, int*, int*", ZERO),
    ("k_unroll_scale_grad", "float const*, float const*, float const*, float*, int, float*", ZERO),
    ("k_unroll_scale_vectors", "lqp::ScaleVecParams", ZERO),
    ("k_unroll_scale_scatter", "float const*, float const*, int const*, int const*, float const*, float*, int", ZERO),
]


def instances():
    """{demangled instance name, e.g. 'lqp::k_pack<float>': its parameter list}, every instance of the manifest"""
    spell = lambda a: str(a).lower() if isinstance(a, bool) else str(a)
    out = {}
    for kernel, sig, arg_tuples in KERNELS:
        for args in arg_tuples:
            name = f"lqp::{kernel}<{', '.join(map(spell, args))}>"
            assert name not in out, name
            out[name] = sig.format(*args)
    return out


def generate():
    """{file name: content} of csrc/split/"""
    by_group = {g: [] for g, _ in GROUPS}
    for n in sorted(f"void {name}({sig})" for name, sig in instances().items()):
        by_group[next(g for g, pred in GROUPS if pred(n))].append(n)
    head = "// generated by tools/gen_split_build.py from the manifest of kernel instances in it -- do not edit\n"
    files = {"lqp_extern.inc": head + "// host translation unit: no kernel of these lists is instantiated here\n" + "".join(
        f"// ---- {g}\n" + "".join(f"extern template __global__ {n};\n" for n in by_group[g]) for g, _ in GROUPS)}
    for g, _ in GROUPS:
        files[f"lqp_tu_{g}.hip"] = head + '#include "../lqp_unroll.hpp"\n' + "".join(f"template __global__ {n};\n" for n in by_group[g])
    return files, {g: len(v) for g, v in by_group.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=OUT, help="directory to write (default: csrc/split)")
    ap.add_argument("--check", action="store_true", help="write nothing; fail when the directory differs from what would be written")
    args = ap.parse_args()
    files, counts = generate()
    if args.check:
        have = {f: open(os.path.join(args.out, f)).read() for f in sorted(os.listdir(args.out))} if os.path.isdir(args.out) else {}
        bad = sorted(f for f in set(files) | set(have) if files.get(f) != have.get(f))
        if bad:
            sys.exit(f"{args.out} is not what tools/gen_split_build.py writes: {', '.join(bad)}")
    else:
        os.makedirs(args.out, exist_ok=True)
        for f, text in files.items():
            with open(os.path.join(args.out, f), "w") as fh:
                fh.write(text)
    print(counts, "kernels:", sum(counts.values()), "translation units:", len(GROUPS), "+ the host's")


if __name__ == "__main__":
    main()
