"""The schedules of the forward solve and of its backward, as data (no GPU needed to import this module).

Every row names one tier the library can select by itself (plan_forward / plan_backward in csrc/lqp_amd.hip) and says how to
reach it: shape, dtype, batch size -- a symbolic expression of the CU count --, control keys and LQP_* environment overrides.
It also says what the forward must report having run (`sig`, compared with sol["_stats"]) and how many iterations the solve is
pinned to (`K`).  tests/test_gpu_tiers.py runs every row on the GPU against the CPU oracle: the truth is the oracle in float64,
the error budget is the oracle in float32 (the same algorithm with LAPACK's rounding), see `compare`.  tests/test_tier_table.py
checks, without a GPU, that the rows cover every schedule-selecting knob and both sides of every size threshold, and that the
comparator can see a one-tile error of 1e-4.  The rows with backward='kkt' compare their gradients with the oracle's KKT-system
backward; tests/kkt_table.py holds that backward's own rows (forms, block counts, one-sided batches).  tests/fp_table.py holds the
fixed-point backward's own rows: synthetic fixed points whose free set has a chosen size, all six gradients.

Row fields:
  name, n, m, dtype ("f32" | "f64"), B (int, or an expression of `cus` such as "cus//4 + 1")
  ctl      control keys on top of the pinned solve: linsolve, launch_mode, sync, rho, scale, backward
  env      LQP_* overrides for this row (set with monkeypatch.setenv; the conftest sets LQP_ENV_NOCACHE=1)
  sig      expected sol["_stats"] entries: linsolve_used, loop_workgroups, factor_launches, mode_used, n_factor
  K        pinned iteration count (eps_abs = eps_rel = 1e-12, max_iters = K + 1): 60, or 250 across adaptive-rho events
  R, F     float32 bar |hip - t64| <= R |t32 - t64| + F scale (defaults 4, 1e-7; ceilings 8, 1e-6 -- raised ones say why in `why`)
  flip     the row runs once more with these overrides instead of `env` ({} = the library's defaults) and asserts that something
           observable changes (stats, per-class launch counts, bits of x or of the gradients): a knob that does not bite fails.
           Rows without env overrides have no flip.
  same     True: the flipped run must give the SAME bits (the knob only moves work between workgroups); `why` says so
  q        "sym" (default) | "nonsym": Q with a small antisymmetric part (the pivoted LU must take it)
"""
import math

import torch

R_DEFAULT, F_DEFAULT = 4.0, 1e-7
R_MAX, F_MAX = 8.0, 1e-6
K_DEFAULT, K_EVENTS = 60, 250
OUTPUTS = ("x", "z", "u", "lams", "nus", "rho")
GRADS = ("dQ", "dp", "dA", "db")

SPD = dict(linsolve_used=2)
LU = dict(linsolve_used=1)


def row(name, n, m, B, dtype="f32", ctl=None, env=None, sig=None, K=K_DEFAULT, R=R_DEFAULT, F=F_DEFAULT, flip=None,
        same=False, q="sym", why=None):
    env = dict(env or {})
    return dict(name=name, n=n, m=m, B=B, dtype=dtype, ctl=dict(ctl or {}), env=env, sig=dict(sig or {}), K=K, R=R, F=F,
                flip=(dict(flip) if flip is not None else ({} if env else None)), same=same, q=q, why=why)


# ---------------------------------------------------------------------------------------------------------------------------------
# expected signatures: loop_workgroups (lw), factor_launches (fl), mode_used (mode)
def sig(base, lw=None, fl=None, mode=None, n_factor=None):
    d = dict(base)
    for k, v in (("loop_workgroups", lw), ("factor_launches", fl), ("mode_used", mode), ("n_factor", n_factor)):
        if v is not None:
            d[k] = v
    return d


def ks(n):
    return (n + 63) // 64


RHO_LO, RHO_HI = dict(rho=0.01), dict(rho=100.0)       # far from the adaptation threshold: whether an event
#                                                         (iterations 100, 200) refactorises is the same in the HIP solve, t32, t64

ROWS = [
    # ---------------- symmetric path, n <= 128: the small loop (k_admm_loop_small, 256 threads, one workgroup) ----------------
    row("small_n1_m0", 1, 0, 3, K=20, sig=sig(SPD, lw=1, fl=1, mode=2),
        why="K = 20: one variable converges exactly (zero residuals) at iteration 25, below any eps"),
    row("small_n31_m1", 31, 1, 4, sig=sig(SPD, lw=1, fl=1, mode=2)),
    row("small_n64_m16", 64, 16, 2, sig=sig(SPD, lw=1, fl=1, mode=2)),
    row("small_n65_m0", 65, 0, 5, sig=sig(SPD, lw=1, fl=1, mode=2)),
    row("small_n128_m1", 128, 1, 3, sig=sig(SPD, lw=1, fl=1, mode=2)),
    row("small_off_n100_m2", 100, 2, 3, env={"LQP_LOOP_SMALL": "0"}, sig=sig(SPD, lw=1, fl=1, mode=2)),
    # ---------------- 128 < n <= 512: the register-resident sweep (one launch) and the split loop ----------------
    row("sweep2_n129_m1", 129, 1, 3, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep2_n255_m2", 255, 2, 4, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep2_n256_m0", 256, 0, 2, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep2_n257_m16", 257, 16, 2, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep4_n448_m1", 448, 1, "cus//4", sig=sig(SPD, lw=4, fl=3, mode=2)),
    row("sweep2_n448_m1", 448, 1, "cus//4 + 1", sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep4_n449_m16", 449, 16, "cus//4", sig=sig(SPD, lw=4, fl=3, mode=2)),
    row("sweep4_n511_m0", 511, 0, 5, sig=sig(SPD, lw=4, fl=3, mode=2)),
    row("sweep4_n512_m2", 512, 2, "cus//4", sig=sig(SPD, lw=4, fl=3, mode=2)),
    row("sweep2_n512_m2", 512, 2, "cus//4 + 1", sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep2_n449_half", 449, 1, "cus//2", sig=sig(SPD, lw=2, fl=3, mode=2)),
    # ... more problems than half the CUs: pairs taking turns (sweep and loop), one launch per check segment
    row("turns_n449_half1", 449, 1, "cus//2 + 1", sig=sig(SPD, lw=2, fl=3, mode=1)),
    row("turns_n330_cus3", 330, 2, "cus + 3", sig=sig(SPD, lw=2, fl=3, mode=1)),
    # ... the one-workgroup sweep (k_spd_inverse) and the multi-launch sweep (one launch per pivot step)
    row("sweep1_n330_turns0", 330, 1, "cus//2 + 1", env={"LQP_SPD_TURNS": "0"}, sig=sig(SPD, lw=2, fl=1, mode=1)),
    row("sweep1_prep_one0", 330, 0, "cus//2 + 1", env={"LQP_SPD_TURNS": "0", "LQP_PREP_ONE": "0"}, sig=sig(SPD, lw=2, fl=1, mode=1),
        flip={"LQP_SPD_TURNS": "0"}),
    row("sweepml_n330_m2", 330, 2, 3, env={"LQP_SPD_RESIDENT": "0", "LQP_SPD_SPLIT": "1"}, sig=sig(SPD, lw=2, fl=ks(330) + 2, mode=2)),
    row("sweep_split0_n200", 200, 1, 3, env={"LQP_SPD_SPLIT": "0"}, sig=sig(SPD, lw=2, fl=1, mode=2)),
    row("sweep_f16off_n449", 449, 1, "cus//4", env={"LQP_SPD_F16": "0"}, sig=sig(SPD, lw=4, fl=3, mode=2)),
    row("sweep_f16off_n200", 200, 16, 3, env={"LQP_SPD_F16": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep_res4off_n500", 500, 1, 8, env={"LQP_SPD_RESIDENT4": "0"}, sig=sig(SPD, lw=4, fl=3, mode=2)),
    row("sweep_qpass0_n330", 330, 1, 4, env={"LQP_QPASS": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep_prep0_n330", 330, 1, 4, env={"LQP_PREP_FUSED": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("sweep_rholate0_n330", 330, 0, 4, env={"LQP_RHO_LATE": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2), same=True,
        why="rho from the sums k_spd_begin leaves rounds to the setup pass's bits here, launches included (measured)"),
    row("sweep_qslazy0_n330", 330, 2, 4, env={"LQP_QS_LAZY": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("eq_in_loop0_n330_m3", 330, 3, 4, env={"LQP_EQ_IN_LOOP": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("noscale_n300", 300, 1, 3, ctl=dict(scale=False), sig=sig(SPD, lw=2, fl=3, mode=2)),
    # ... the loop: split off, four workgroups off, pairs-taking-turns off
    row("loop_split0_n330", 330, 1, 4, env={"LQP_LOOP_SPLIT": "0"}, sig=sig(SPD, lw=1, fl=3, mode=2)),
    row("loop_split4off_n500", 500, 0, "cus//4", env={"LQP_LOOP_SPLIT4": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("loop_seg0_n330", 330, 2, "cus//2 + 1", env={"LQP_LOOP_SPLIT_SEG": "0"}, sig=sig(SPD, lw=1, fl=3, mode=2)),
    # ... launch modes, the host-driven plan, the un-synchronised module path
    row("mode1_n330", 330, 1, 4, ctl=dict(launch_mode=1), sig=sig(SPD, lw=1, fl=3, mode=1)),
    row("env_mode1_n200", 200, 2, 3, env={"LQP_LAUNCH_MODE": "1"}, sig=sig(SPD, lw=1, fl=3, mode=1)),
    row("mode2_nosync_n330", 330, 2, 3, ctl=dict(launch_mode=2, sync=False), sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("syncplan0_n330", 330, 1, 3, env={"LQP_SYNC_PLAN": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2), same=True,
        why="host-driven chunks enqueue the same kernels on the same data as the up-front plan"),
    row("env_lu_n330", 330, 1, 3, env={"LQP_LINSOLVE": "1"}, sig=sig(LU, fl=2, mode=2)),
    # ... adaptive-rho events (K = 250: events at 100 and 200)
    row("events_lo_n330", 330, 1, 4, ctl=RHO_LO, K=K_EVENTS, sig=sig(SPD, lw=2, fl=3, mode=2, n_factor=2)),
    row("events_hi_n449_mode1", 449, 2, 3, ctl=dict(RHO_HI, launch_mode=1), K=K_EVENTS, sig=sig(SPD, lw=1, fl=3, mode=1, n_factor=3)),
    row("events_small_n100", 100, 1, 4, ctl=RHO_HI, K=K_EVENTS, sig=sig(SPD, lw=1, fl=1, mode=2, n_factor=3)),
    row("events_hotpast0", 330, 1, 4, ctl=RHO_LO, K=K_EVENTS, env={"LQP_HOT_PAST": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2, n_factor=2)),
    row("events_hotrounds0", 330, 1, 4, ctl=RHO_LO, K=K_EVENTS, env={"LQP_HOT_ROUNDS": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2, n_factor=2)),
    row("events_tailepi0", 330, 1, 4, ctl=RHO_LO, K=K_EVENTS, env={"LQP_TAIL_EPILOGUE": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2, n_factor=2)),
    row("events_nosyncmax0", 330, 1, 4, ctl=RHO_LO, K=K_EVENTS, env={"LQP_NOSYNC_MAX_EVENTS": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2, n_factor=2)),
    row("events_turns", 330, 1, "cus//2 + 1", ctl=RHO_HI, K=K_EVENTS, sig=sig(SPD, lw=2, fl=3, mode=1, n_factor=3)),
    # ---------------- 512 < n <= 1024: two workgroups per matrix (two steps per pass) and the streaming loop ----------------
    row("big_n513_m2", 513, 2, 3, sig=sig(SPD, lw=2, fl=2 * ks(513) + 2, mode=2)),
    row("big_n576_m0", 576, 0, 2, sig=sig(SPD, lw=2, fl=2 * ks(576) + 2, mode=2)),
    row("big_n1000_m1", 1000, 1, 2, sig=sig(SPD, lw=2, fl=2 * ks(1000) + 2, mode=2)),
    row("big_n1023_m0", 1023, 0, 2, sig=sig(SPD, lw=2, fl=2 * ks(1023) + 2, mode=2)),
    row("big_n1024_m1", 1024, 1, 2, sig=sig(SPD, lw=2, fl=2 * ks(1024) + 2, mode=2)),
    row("big_fuse0_n700", 700, 1, 2, env={"LQP_SPD_BIG_FUSE": "0"}, sig=sig(SPD, lw=2, fl=2 * ks(700) + 2, mode=2)),
    row("big_fuse0_same_as_f16off", 700, 1, 2, env={"LQP_SPD_BIG_FUSE": "0"}, flip={"LQP_SPD_BIG_F16": "0"}, same=True,
        sig=sig(SPD, lw=2, fl=2 * ks(700) + 2, mode=2),
        why="one launch pair per step and the fused float32 steps are the same operations in the same order"),
    row("big_f16off_n1000", 1000, 4, 2, env={"LQP_SPD_BIG_F16": "0"}, sig=sig(SPD, lw=2, fl=2 * ks(1000) + 2, mode=2)),
    row("big_np2off_n1000", 1000, 1, 3, env={"LQP_LOOP_NP2": "0"}, sig=sig(SPD, lw=1, fl=2 * ks(1000) + 2, mode=2)),
    row("big_one_wg_n600", 600, 1, 2, env={"LQP_SPD_SPLIT": "0"}, sig=sig(SPD, lw=2, fl=1, mode=2)),
    row("big_many_n600", 600, 0, "cus//2 + 1", sig=sig(SPD, lw=1, fl=1, mode=2)),
    row("big_off_n600", 600, 1, 2, env={"LQP_SPD_BIG": "0"}, sig=sig(LU, fl=2, mode=2)),
    row("big_mode1_n800", 800, 2, 2, ctl=dict(launch_mode=1), sig=sig(SPD, lw=1, fl=2 * ks(800) + 2, mode=1)),
    # ---------------- the LU path ----------------
    # m = 17 leaves the symmetric path; a non-symmetric Q too
    row("lu_m17_n200", 200, 17, 3, sig=sig(LU, lw=2, fl=2, mode=2)),
    row("lu_m16_n200", 200, 16, 3, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("lu_nonsym_n300", 300, 1, 3, q="nonsym", sig=sig(LU, fl=2, mode=2)),
    row("lu_nonsym_n200_f64", 200, 2, 3, dtype="f64", q="nonsym", sig=sig(LU, lw=2, fl=2, mode=2)),
    # one-workgroup LU with cached triangular solves (segmented launches keep the dense tiers out)
    row("lu1_n300_f32", 300, 2, 3, ctl=dict(linsolve="lu", launch_mode=1), env={"LQP_LU2": "0"}, sig=sig(LU, lw=1, fl=2, mode=1),
        same=True, why="the two-workgroup LU gives the one-workgroup kernel's bits in float32 (test_two_workgroup_lu)"),
    row("lu1_mfma0_n500_f32", 500, 1, 3, ctl=dict(linsolve="lu", launch_mode=1), env={"LQP_LU2": "0", "LQP_LU_MFMA": "0"},
        flip={"LQP_LU2": "0"}, sig=sig(LU, lw=1, fl=2, mode=1), same=True,
        why="the trailing update on the matrix cores rounds as the vector unit's does: the same bits (measured)"),
    row("lu1_mfma0_n700_f32", 700, 0, 2, ctl=dict(linsolve="lu", launch_mode=1), env={"LQP_LU_MFMA": "0"}, sig=sig(LU, lw=1, fl=2, mode=1),
        same=True, why="the trailing update on the matrix cores rounds as the vector unit's does: the same bits (measured)"),
    row("lu1_n300_f64", 300, 2, 3, dtype="f64", ctl=dict(launch_mode=1), env={"LQP_LU2": "0"}, sig=sig(LU, lw=1, fl=2, mode=1)),
    row("lu1_resident0_n130_f64", 130, 1, 2, dtype="f64", ctl=dict(launch_mode=1), env={"LQP_LU2": "0", "LQP_RESIDENT": "0"},
        flip={"LQP_LU2": "0"}, sig=sig(LU, lw=1, fl=2, mode=1), same=True,
        why="where the loop keeps the head of the factor (registers / LDS or memory) does not change its arithmetic"),
    row("lu2_n450_f32", 450, 3, 4, ctl=dict(linsolve="lu", launch_mode=1), sig=sig(LU, lw=1, fl=2, mode=1)),
    row("lu2_n450_f64", 450, 3, 4, dtype="f64", ctl=dict(launch_mode=1), sig=sig(LU, lw=1, fl=2, mode=1)),
    row("lu_many_n300_f64", 300, 1, "cus//2 + 1", dtype="f64", sig=sig(LU, lw=1, fl=2)),
    row("lu_mode2_f32_cus", 200, 2, "cus//2 + 1", ctl=dict(linsolve="lu", launch_mode=2), sig=sig(LU, lw=1, fl=2, mode=2)),
    # the dense tier (explicit inverse in registers): n <= 256 on two workgroups, on W workgroups above
    row("dense_n200_f32", 200, 3, 4, ctl=dict(linsolve="lu"), sig=sig(LU, lw=2, fl=2, mode=2)),
    row("dense_n256_f64", 256, 2, 3, dtype="f64", sig=sig(LU, lw=2, fl=2, mode=2)),
    row("densew_n257_f64", 257, 2, 3, dtype="f64", sig=sig(LU, fl=2, mode=2)),
    row("densew_n400_f32", 400, 1, 3, ctl=dict(linsolve="lu"), sig=sig(LU, fl=2, mode=2)),
    row("dense_off_n200_f64", 200, 1, 3, dtype="f64", env={"LQP_LOOP_DENSE": "0"}, sig=sig(LU, lw=1, fl=2, mode=2)),
    row("densew_off_n400_f64", 400, 1, 3, dtype="f64", env={"LQP_LOOP_DENSE_W": "0"}, sig=sig(LU, lw=1, fl=2, mode=2)),
    row("dense_nosync_f64", 120, 2, 3, dtype="f64", ctl=dict(sync=False), sig=sig(LU, lw=2, fl=2, mode=2)),
    row("dense_chunked_f64", 120, 2, 3, dtype="f64", env={"LQP_SYNC_PLAN": "0"}, sig=sig(LU, lw=2, fl=2, mode=2), same=True,
        why="host-driven chunks enqueue the same kernels on the same data as the schedule enqueued up front"),
    # above 1024 rows: the wide LU (#CUs / B workgroups per matrix) and the big LU (two panel rows per thread)
    row("wide_n1025_f32", 1025, 0, 2, sig=sig(LU, fl=2, mode=2)),
    row("bigl_n1025_f32", 1025, 0, 2, env={"LQP_LU_WIDE": "0"}, sig=sig(LU, fl=2, mode=2), same=True,
        why="float32: the wide LU gives the big LU's factor bit for bit (test_lu_wide_matches_one_workgroup)"),
    row("wide_n2048_f32", 2040, 8, 2, sig=sig(LU, fl=2, mode=2)),
    row("wide_n2049_f32", 2049, 0, 1, sig=sig(LU, fl=2, mode=2)),
    row("bigl_n2049_f32", 2049, 0, 1, env={"LQP_LU_WIDE": "0"}, sig=sig(LU, fl=2, mode=2), same=True,
        why="float32: the wide LU gives the big LU's factor bit for bit (test_lu_wide_matches_one_workgroup)"),
    row("bigl_n1100_f64", 1100, 2, 2, dtype="f64", env={"LQP_LU_WIDE": "0"}, sig=sig(LU, fl=2, mode=2), same=True,
        why="float64 at B = 2: the wide LU's factor gives the big LU's iterates bit for bit (measured)"),
    row("wide_n1100_f64", 1100, 2, 2, dtype="f64", sig=sig(LU, fl=2, mode=2)),
    row("wide_n2047_f64", 2047, 0, 1, dtype="f64", sig=sig(LU, fl=2, mode=2)),
    row("lu_events_n300_f64", 300, 1, 3, dtype="f64", ctl=RHO_HI, K=K_EVENTS, sig=sig(LU, fl=2, mode=2, n_factor=2)),
    row("lu_events_n200_f32", 200, 17, 3, ctl=dict(RHO_LO, launch_mode=1), K=K_EVENTS, sig=sig(LU, lw=1, fl=2, mode=1, n_factor=2)),
    # ---------------- backward forms (the module path: the prefactored Cholesky form after the symmetric x-update) ----------------
    row("bwd_f16off_n330", 330, 1, 4, env={"LQP_BWD_F16": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("bwd_la0_n449_m3", 449, 3, 4, env={"LQP_BWD_LOOKAHEAD": "0"}, sig=sig(SPD, lw=4, fl=3, mode=2)),
    row("bwd_equil0_n330_m2", 330, 2, 4, env={"LQP_BWD_EQUIL": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("bwd_chol0_n330", 330, 2, 4, env={"LQP_BWD_CHOL": "0"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("bwd_refine0_lu_n200", 200, 2, 3, ctl=dict(linsolve="lu"), env={"LQP_BWD_REFINE": "0"}, sig=sig(LU, lw=2, fl=2, mode=2)),
    row("bwd_refine0_lu_f64", 150, 3, 3, dtype="f64", env={"LQP_BWD_REFINE": "0"}, sig=sig(LU, lw=2, fl=2, mode=2)),
    row("bwd_split2off_lu_n200", 200, 2, 3, ctl=dict(linsolve="lu"), env={"LQP_SPLIT2": "0"}, sig=sig(LU, lw=2, fl=2, mode=2), same=True,
        why="the second workgroup per problem takes whole rows of the pack / build / residual kernels: the same bits (measured)"),
    row("bwd_full_n200", 200, 2, 3, env={"LQP_BWD_FULL": "1"}, sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("bwd_full_lu_f64", 150, 1, 3, dtype="f64", env={"LQP_BWD_FULL": "1"}, sig=sig(LU, lw=2, fl=2, mode=2)),
    row("bwd_kkt_n200", 200, 2, 3, ctl=dict(backward="kkt"), sig=sig(SPD, lw=2, fl=3, mode=2)),
    row("bwd_kkt_lu_f64", 150, 2, 3, dtype="f64", ctl=dict(backward="kkt"), sig=sig(LU, lw=2, fl=2, mode=2)),
]

ROW_BY_NAME = {r["name"]: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS), "duplicate row names"

# ---------------------------------------------------------------------------------------------------------------------------------
# knobs of docs/KNOBS.md that no row has to force, each with its reason (tests/test_tier_table.py: every other knob needs a row)
NOT_A_TIER = {
    "LQP_DBG_LOOP_ABSENT": "debug: makes a shared kernel wait for a partner that never comes (fault-path tests)",
    "LQP_DBG_LU2_ABSENT": "debug: the two-workgroup LU without its partner (fault-path tests)",
    "LQP_DBG_QPASS": "debug stamps of the resident sweep",
    "LQP_DBG_SETUP": "debug stamps of the setup kernel",
    "LQP_LOOP512": "measurement only: the 512-thread build of the one-workgroup loop, measured slower",
    "LQP_SYM512": "measurement only: the 512-thread build of the symmetric one-workgroup loop, measured slower",
    "LQP_LU_NT": "measurement only: thread count of the one-workgroup LU",
    "LQP_LU_PB": "measurement only: panel width of the one-workgroup LU",
    "LQP_LU_WIDE_MIN": "measurement only: the row count above which the wide LU is tried (LQP_LU_WIDE selects the tier)",
    "LQP_SPEC_LAUNCHES": "measurement only: check segments enqueued speculatively per host round trip",
    "LQP_XCD_LOCAL": "transport: how partner workgroups exchange (test_xcd_local_exchange_is_only_a_transport: same bits)",
    "LQP_INV_XCD": "transport: which XCD the inverse's column tiles run on",
    "LQP_EPI_SLABS": "transport: row slabs of the backward epilogue (each row is computed whole either way)",
    "LQP_BWD_EARLY": "transport: which launch reports the backward's info words",
    "LQP_SPD_PTASKS": "transport: tile tasks handed between the workgroups of the multi-launch sweep",
    "LQP_UNROLL_EVENTS": "unroll=True only: tests/unroll_table.py holds its rows (tests/test_unroll_table.py requires one per value)",
    "LQP_UNROLL_SPLIT": "unroll=True only: tests/unroll_table.py holds its rows (tests/test_unroll_table.py requires one per value)",
    "LQP_UNROLL_NATIVE": "unroll=True only: tests/unroll_table.py holds its rows (tests/test_unroll_table.py requires one per value)",
    "LQP_UNROLL_SCALE_NATIVE": "unroll=True only: tests/unroll_table.py holds its rows (tests/test_unroll_table.py requires one per value)",
}

# size thresholds of the selection code: (what, row predicate of the lower side, of the upper side)
THRESHOLDS = {
    "n 128 | 129 (SPLIT_MINK)": ("n", 128, 129),
    "n 256 | 257 (dense tier)": ("n", 256, 257),
    "n 512 | 513 (SPD_MAXK)": ("n", 512, 513),
    "n 1024 | 1025 (SPD_BIGK, wide LU)": ("n", 1024, 1025),
    "N 2048 | 2049": ("N", 2048, 2049),
    "m 16 | 17": ("m", 16, 17),
    "B cus/4 | cus/4 + 1": ("B", "cus//4", "cus//4 + 1"),
    "B cus/2 | cus/2 + 1": ("B", "cus//2", "cus//2 + 1"),
}


def batch(r, cus):
    B = r["B"]
    if isinstance(B, int):
        return B
    return int(eval(B, {"__builtins__": {}}, {"cus": int(cus)}))


def sample(B):
    """Problems compared against the CPU oracle: all of a batch up to 8, else four of them, the first and the last among them."""
    if B <= 8:
        return list(range(B))
    return sorted({0, B // 3, (2 * B) // 3, B - 1})


def seed_of(r):
    """(`j`: the offset a row of tests/unroll_table.py found by its seed search; the rows of this table have none)"""
    return sum(ord(c) * (i + 1) for i, c in enumerate(r["name"])) % 100003 + r.get("j", 0)


def _problem(r, i, qcache=None):
    """Problem i of the row's batch, float64: Q from one of a few draws (cheap at large batches), p / bounds / A per problem, with
    the input edges: some lb = -inf, some ub = +inf, a few lb == ub, active and inactive bounds, random A rows."""
    n, m = r["n"], r["m"]
    s = seed_of(r)
    Q = None if qcache is None else qcache.get(i % 5)
    if Q is None:
        gq = torch.Generator().manual_seed(s * 7 + (i % 5))
        G = torch.randn(n + 8, n, generator=gq, dtype=torch.float64)
        Q = G.T @ G / (n + 8) + 0.05 * torch.eye(n, dtype=torch.float64)
        if r["q"] == "nonsym":
            S = torch.randn(n, n, generator=gq, dtype=torch.float64)
            Q = Q + 0.02 * (S - S.T)
        else:
            Q = 0.5 * (Q + Q.T)
        if qcache is not None:
            qcache[i % 5] = Q
    g = torch.Generator().manual_seed(s * 7919 + i)
    p = torch.randn(n, 1, generator=g, dtype=torch.float64)
    lb = -(1.0 + torch.rand(n, 1, generator=g, dtype=torch.float64))
    ub = 1.0 + torch.rand(n, 1, generator=g, dtype=torch.float64)
    if n >= 6:
        lb[1::7] = -math.inf
        ub[3::11] = math.inf
        fixed = torch.arange(5, n, 37)
        c = 0.5 * torch.rand(len(fixed), 1, generator=g, dtype=torch.float64) - 0.25
        lb[fixed] = c
        ub[fixed] = c
    A = b = None
    if m:
        A = torch.randn(m, n, generator=g, dtype=torch.float64)
        x0 = torch.maximum(torch.minimum(0.3 * torch.randn(n, 1, generator=g, dtype=torch.float64), ub), lb)
        b = A @ x0
    return Q, p, A, b, lb, ub


def inputs(r, B, idx=None):
    """(Q, p, A, b, lb, ub) of the batch -- or of the problems `idx` of it -- in the row's dtype."""
    dt = torch.float32 if r["dtype"] == "f32" else torch.float64
    idx = range(B) if idx is None else idx
    qcache = {}
    parts = [_problem(r, i, qcache) for i in idx]
    out = []
    for k in range(6):
        if parts[0][k] is None:
            out.append(None)
        else:
            out.append(torch.stack([pt[k] for pt in parts]).to(dt))
    return tuple(out)


def control(r, **extra):
    """The oracle's control for the pinned solve of row r (the HIP call adds linsolve / launch_mode / sync / backward)."""
    c = dict(eps_abs=1e-12, eps_rel=1e-12, max_iters=r["K"] + 1)
    for k in ("rho", "scale"):
        if k in r["ctl"]:
            c[k] = r["ctl"][k]
    c.update(extra)
    return c


def oracle(r, inp, dtype, cot=None):
    """The CPU oracle's pinned solve of `inp` in `dtype` (and its fixed-point gradient of the cotangent `cot`)."""
    from oracle import boxqp_oracle as O
    d = [None if t is None else t.to(dtype) for t in inp]
    trace = {}
    sol = O.solve_box_qp(*d, O.make_control(**control(r)), trace=trace)
    sol["n_factor"] = trace["n_factor"]
    if cot is not None:
        g = O.solve_box_qp_grad(cot.to(dtype), sol["x"], sol["u"], sol["lams"], sol["nus"], d[0], d[2], d[4], d[5], sol["rho"])
        sol["grads"] = dict(zip(("dQ", "dp", "dA", "db", "dlb", "dub"), g[:6]))
    return sol


def _as_tensor(v, like):
    if torch.is_tensor(v):
        return v.detach().cpu().double()
    return torch.full((like.shape[0], 1, 1), float(v), dtype=torch.float64)


def compare(r, hip, t32, t64, keys=OUTPUTS):
    """The row's bar for each output: float32 rows |hip - t64| <= R |t32 - t64| + F scale, float64 rows |hip - t64| <= 1e-9 scale,
    scale = max(1, |t64|_inf), every norm the largest absolute entry over the compared problems.  Returns {key: record} -- each
    record holds the errors, the ratio |hip - t64| / |t32 - t64| and `ok`."""
    out = {}
    like = next(v for v in t64.values() if torch.is_tensor(v) and v.dim() == 3)
    for k in keys:
        if t64.get(k) is None or hip.get(k) is None:
            continue
        ref = _as_tensor(t64[k], like)
        h = _as_tensor(hip[k], like)
        scale = max(1.0, float(ref.abs().max()))
        e_hip = float((h - ref).abs().max())
        rec = dict(err=e_hip, scale=scale)
        if r["dtype"] == "f64":
            rec.update(bar=1e-9 * scale, ok=e_hip <= 1e-9 * scale)
        else:
            e32 = float((_as_tensor(t32[k], like) - ref).abs().max())
            bar = r["R"] * e32 + r["F"] * scale
            rec.update(budget=e32, ratio=e_hip / e32 if e32 > 0 else (0.0 if e_hip == 0 else math.inf), bar=bar, ok=e_hip <= bar)
        out[k] = rec
    return out


def perturb_last_block(Q):
    """Q with its last (partial) diagonal 64-block scaled by 1 + 1e-4, kept symmetric: the one-tile error the GPU module must see."""
    n = Q.shape[-1]
    s = ((n - 1) // 64) * 64
    Q = Q.clone()
    Q[:, s:, s:] *= 1 + 1e-4
    return Q
