/*
 * lqp_amd.h -- C ABI of the MI355X-native batched box-QP ADMM layer.
 *
 * The reference (ipo-lab/lqp_py) has no FFI: its boundary is a Python API on
 * top of torch.linalg.  Each entry point below replaces the reference call
 * sites listed next to it; the Python shim in lqp_py_amd/ binds them with
 * ctypes and keeps the reference's signatures.
 *
 * Conventions
 *   - every function returns an int status (LQP_OK == 0), never throws,
 *     never allocates: scratch comes from the caller (`workspace`), sized by
 *     the matching *_workspace_bytes query;
 *   - all tensor pointers are DEVICE pointers to dense, batch-first,
 *     row-major (C-contiguous) arrays, exactly the layout of a contiguous
 *     torch tensor of the stated shape; every vector, matrix and workspace
 *     pointer is 16-byte aligned (the kernels take 16-byte loads and stores
 *     where a row length allows; the Python shim copies a tensor that is
 *     not), arrays of one scalar per problem (rho, beta, info, iteration
 *     counts) need the alignment of their element only;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - dtype: LQP_F32 or LQP_F64 (the arithmetic type of every tensor).
 */
#ifndef LQP_AMD_H
#define LQP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LQP_ABI_VERSION 17

enum { LQP_F32 = 0, LQP_F64 = 1 };

enum {
    LQP_OK = 0,
    LQP_ERR_INVALID = 1,      /* bad argument (null pointer, negative size, unknown dtype) */
    LQP_ERR_WORKSPACE = 2,    /* workspace smaller than *_workspace_bytes               */
    LQP_ERR_SINGULAR = 3,     /* exactly-zero pivot; batch index in stats / info         */
    LQP_ERR_HIP = 4,          /* a HIP runtime call failed                               */
    LQP_ERR_TIMEOUT = 5,      /* in-kernel grid barrier gave up (bounded spin)           */
    LQP_ERR_UNSUPPORTED = 6,  /* size outside what the kernels are built for: n + m > 4096 (float32) / 2048 (float64) */
    LQP_ERR_NOT_SPD = 7       /* lqp_boxqp_forward_finish only: the matrix left the symmetric x-update (not symmetric / Qs + rho I not
                                 positive definite in f32): repeat lqp_boxqp_forward with ctrl.linsolve = 1                     */
};

/* Resolved solver controls.  Key-name resolution of the reference's control
 * dict (lqp_py/solve_box_qp_admm_torch.py:133-154, lqp_py/control.py:1-24) and
 * the dict side effect (:37-38) stay in the Python shim; this struct carries
 * the numbers the loop actually uses. */
typedef struct lqp_boxqp_ctrl {
    int32_t max_iters;
    int32_t check_solved;            /* convergence test every this many iterations   */
    int32_t adaptive_rho;            /* 0/1                                            */
    int32_t adaptive_rho_iter;       /* already rounded to a multiple of check_solved */
    int32_t adaptive_rho_max_iter;
    int32_t scale;                   /* 0/1 auto-scaling (:160-197)                    */
    int32_t any_lb;                  /* not read since ABI 5: whether max(lb) > -inf / min(ub) < +inf over the batch  */
    int32_t any_ub;                  /* (:129-130) is found on the DEVICE (the clamps always run -- an infinite bound
                                        is an exact no-op -- and the answer comes back in lqp_boxqp_stats.any_lb/ub
                                        or, for un-synchronised calls, in status words 12/13).  What the caller must
                                        still decide itself is the reference's rho = 0 shortcut for a batch without any
                                        finite bound (:157-158): pass rho_mode 1, rho_value 0 for it.              */
    int32_t rho_mode;                /* 0 auto (||Q||_F/sqrt(n), :200-203), 1 scalar rho_value,
                                        2 per-problem array `rho_in` (B values)        */
    int32_t beta_mode;               /* 0 auto (quantile rule :171-174), 1 scalar beta_value, 2 per-problem array
                                        `beta_in` (B values; the reference accepts a (B,1) tensor, :171-175)  */
    int32_t launch_mode;             /* 0 auto, 1 one launch per check segment,
                                        2 persistent loop kernel with in-kernel grid barrier */
    int32_t reserved;                /* 1: do not synchronise with the host (needs persistent launches and a
                                        short adaptive-rho schedule, else ignored): the whole schedule is
                                        enqueued speculatively, stats come back as -1, and the caller fetches
                                        status / info later (lqp_boxqp_forward_layout)
                                        2: split synchronous call (needs host_report): the schedule is enqueued
                                        and the call returns with stats.mode_used = 4; the caller does its own
                                        host work while the GPU runs and then calls lqp_boxqp_forward_finish,
                                        which waits and reports like a synchronous call would have.  Where the
                                        library cannot enqueue the whole schedule (segmented launches, a check
                                        hook) the call simply waits itself (mode_used 1 / 2)                  */
    int32_t linsolve;                /* x-update linear algebra: 0 auto, 1 pivoted LU of the KKT matrix (the
                                        reference's, :214-215/:267), 2 symmetric inverse of Qs + rho I with a
                                        rank-m equality correction (f32, n <= 1024, m <= 16, rho > 0; anything
                                        else, or a matrix that is not positive definite, runs on LU)            */
    int32_t reserved2;               /* bit 0: leave the complete factor (equality correction included) in the workspace for
                                        lqp_boxqp_unroll_backward; bit 1 (ABI 11): share nothing between workgroups -- one
                                        workgroup per matrix everywhere, host-launched check segments: what the library falls
                                        back to by itself when a kernel that waits for a partner workgroup gives up (CUs held
                                        by another stream / process), and what a caller of lqp_boxqp_forward_finish that got
                                        LQP_ERR_TIMEOUT passes when it repeats the forward; bit 2 (ABI 12): keep a
                                        trace of the convergence checks -- the largest primal and dual error over the batch at
                                        every check, what the reference prints under verbose=True (:289-294) -- for
                                        lqp_boxqp_check_trace; bit 3 (ABI 14): the problems are independent -- every
                                        problem is solved as the reference would solve it in a batch of one: it stops at the
                                        first check at which IT is optimal and adapts rho from its own residual ratio, so its
                                        result does not depend on what else is in the batch.  stats.iters and status word [1]
                                        then carry the largest per-problem count; lqp_boxqp_problem_iters copies out all of
                                        them.  Not with check_hook (LQP_ERR_INVALID)                                     */
    double eps_abs;
    double eps_rel;
    double rho_value;
    double rho_min;
    double rho_max;
    double adaptive_rho_tol;
    double adaptive_rho_threshold;
    double beta_value;
    const void* beta_in;             /* beta_mode == 2: B values of the tensors' dtype (device pointer), else NULL */
    /* Strict global stopping across batch shards (one process per GPU): when set, the solve runs one
     * launch per check segment and, right after the launch that holds check number `check_index`, calls
     *     check_hook(check_hook_user, stream, counters, check_index)
     * on the host with the DEVICE address of that check's FOUR uint32 words {problems not yet optimal, arrivals
     * (unused in this mode), problems that want a rho update, problems whose residual ratio triggers one} (:310-312,
     * :244-246).  The hook must enqueue, ordered on `stream`, an in-place SUM all-reduce of all four words over the
     * ranks (RCCL); every consumer of the counters (stop test, adaptive-rho decision) is enqueued after it, so all
     * ranks take the single-process decisions and report the single-process iteration count.
     * check_index == -1: the same reduction over the four-word failure vote of a factorisation {ranks whose matrix
     * left the symmetric x-update, ranks with an exactly singular KKT matrix, 0, 0}: every rank then repeats the solve
     * on the LU path, or fails, together -- the sequence of collectives stays the same on all ranks.
     * Non-zero return aborts the solve (LQP_ERR_HIP).  NULL: decisions are per call (per shard).                  */
    int (*check_hook)(void* user, void* stream, void* counters_dev, int check_index);
    void* check_hook_user;
    const void* bound_flags_in;      /* optional: two int32 on the device {any_lb, any_ub} of a LARGER batch this call
                                        holds one shard of (one all-reduce MAX over the ranks); they are
                                        OR-ed into the answer reported back.  NULL: this call is the whole batch.    */
    void* host_report;               /* optional: PINNED host memory the device can write (hipHostMalloc /
                                        torch pin_memory), 16 + 2 B int32.  The forward's last kernel then leaves
                                        there, with no device-to-host copy: [0..16) the status block (see
                                        lqp_boxqp_forward_layout), [16..16+B) the info word of every problem,
                                        [16+B..16+2B) per-problem flag bits {1: a lower bound is finite, 2: an upper
                                        bound is finite, 4: its workgroup saw a barrier timeout, 8: its matrix left the
                                        symmetric x-update, 65536 (bit 16, added within ABI 17): flagged primal
                                        infeasible by lqp_boxqp_forward_detect / _certify, 131072 (bit 17, added within
                                        ABI 17): flagged dual infeasible by lqp_boxqp_forward_certify}.  Valid once the stream has passed the call (an event):
                                        ctrl.reserved = 1 callers read it then.  A synchronous call sets every
                                        word to -1 before its first launch and POLLS them (all stored words are >= 0)
                                        instead of synchronising the stream: it returns about a microsecond after the
                                        last kernel's stores, not after an interrupt-driven stream wait.            */
    double alpha;                    /* ABI 17, appended (every earlier offset holds): over-relaxation of the ADMM step.  The
                                        z- and the dual update of an iteration see alpha x + (1 - alpha) z_prev in place of
                                        x; the residuals of the check, the next right-hand side and the returned x do not
                                        change, and the fixed point (x = z) is the same.  0 = not set = 1 (the reference's
                                        plain step; a zero-initialised struct keeps it); otherwise finite and inside (0, 2),
                                        and 1 whenever reserved2 bit 0 is set (the unrolled backward replays the plain
                                        step): LQP_ERR_INVALID else.  Ignored by the rho = 0 one-shot, which does not
                                        iterate.                                                                        */
} lqp_boxqp_ctrl;

/* Host-side bookkeeping returned by the forward solve. */
typedef struct lqp_boxqp_stats {
    int32_t iters;          /* == the reference's sol["iter"]                          */
    int32_t n_factor;       /* LU factorisations (1 + adaptive-rho refactors)          */
    int32_t n_solve;        /* x-updates == iters + 1                                  */
    int32_t n_check;        /* convergence checks performed                            */
    int32_t rho_updated;    /* 1 if adaptive rho changed rho at least once             */
    int32_t fail_index;     /* batch index of the first singular problem, or -1        */
    int32_t n_launch;       /* kernel launches issued                                  */
    int32_t mode_used;      /* 1 segmented, 2 persistent, 3 persistent without host sync, 4 enqueued, lqp_boxqp_forward_finish pending */
    int32_t linsolve_used;  /* 1 pivoted LU, 2 symmetric inverse (what linsolve 0 / a fallback resolved to) */
    int32_t factor_launches; /* kernel launches per (re)factorisation: 1, 2 (LU + pack) or Ks + 2 when a small batch
                              * shares each matrix between two workgroups (one launch per pivot step) */
    int32_t loop_workgroups; /* workgroups per QP in the first (hot) loop launch: 1, 2 (2 B <= CUs) or 4 (4 B <= CUs) when a small batch
                              * on the symmetric path splits every product between two CUs */
    int32_t any_lb;          /* 1: some lower bound of the batch is finite (:129), 0: none, -1: not known on the host */
    int32_t any_ub;          /* the same for the upper bounds (:130)                                                 */
    int32_t loop_kind;       /* (ABI 14) the kernel family of the first (hot) loop launch: 0 one workgroup per QP, 1 the split loop
                              * (two / four workgroups, matrix in registers; also its turn-taking segments), 2 the small loop
                              * (n <= 128), 3 two streaming workgroups (n > 512), 4 / 5 the dense LU-tier loops        */
} lqp_boxqp_stats;

int lqp_abi_version(void);
/* ABI 17: sizeof(lqp_boxqp_ctrl) as this library was built -- a caller whose struct is shorter was built against an older header */
size_t lqp_boxqp_ctrl_bytes(void);
const char* lqp_status_string(int status);

/* ---- measurement hooks (not part of the reference surface) ----------------
 * When enabled, every kernel launch issued by this library is bracketed by a
 * pair of HIP events recorded on the launch stream; lqp_profile_get waits for
 * them and returns, per kernel class, the summed device time in ms and the
 * launch count since the last reset.  bench.py uses this for the roofline. */
void lqp_profile_enable(int on);
void lqp_profile_reset(void);
int lqp_profile_classes(void);
const char* lqp_profile_class_name(int cls);
int lqp_profile_get(double* total_ms, long long* launches, int n);
/* debug: device buffer of 4 uint64 per problem; every LU launch then writes its shader-clock
 * cycles spent in (panel, swaps+U12, trailing update, total).  NULL switches it off. */
void lqp_debug_set_lu_counters(void* device_buf);
/* test aid: occupies `blocks` workgroups (512 threads, `lds_bytes` of LDS each) for `usec` microseconds on `stream`:
 * the co-residency tests run the two-workgroup schedules of the forward solve beside it. */
int lqp_debug_spin(void* stream, int blocks, int usec, int lds_bytes);
/* test aid: out_dev[b] (int32, device) := the XCD (0..7, HW_REG_XCC_ID) workgroup b of a `blocks`-workgroup launch runs on --
 * the question the workgroups that share a matrix ask at every launch before they choose their exchange protocol.        */
int lqp_debug_xcd(void* stream, int blocks, void* out_dev);
/* test access to the dense tier's first kernel (csrc/lqp_dense.hpp): X (B, N, N) = M^-1 from a packed factor
 * (`packed`: the buffer lqp_lu_pack filled).  Any N whose column tile fits the LDS: float32 to 2048 (above 576 rows on 16-column
 * tiles), float64 to about 1100; LQP_ERR_UNSUPPORTED beyond.  No reference counterpart. */
int lqp_debug_lu_inverse(void* stream, int dtype, int B, int N, const void* packed, void* X_out);
/* test access to the block solves of the Cholesky backward (csrc/lqp_spd.hpp; ABI 15): L L^T X = V, float32, one workgroup per
 * problem.  `packed`: B factors of sym_blocks(Kmax) = Kmax (Kmax + 1) / 2 blocks of 64 x 64 each, problem b's own kb[b] <= Kmax
 * block rows laid out as the backward lays them out (lower blocks column by column, block (i, j) at j kb - j (j - 1) / 2 + i - j,
 * row-major inside a block, diagonal blocks holding the INVERSE of L's diagonal block); kb: B int32 on the device; V, X_out:
 * (B, nrhs, 64 Kmax), X_out zero past 64 kb[b].  nr = 2 | 4 right-hand sides per round; which = 0: wg_chol_solve_n whatever
 * kb[b], 1: what k_bwd_chol_solve calls (the register-resident solve up to its block limit, wg_chol_solve_n above).
 * Kmax <= 8, nrhs <= 32.  No reference counterpart. */
int lqp_debug_chol_solve(void* stream, int B, int Kmax, const void* packed, const void* kb, int nrhs, int nr, int which,
                         const void* V, void* X_out);
/* test access to the factorisation of the Cholesky backward (csrc/lqp_spd.hpp; ABI 16): in place on `packed_inout`, B matrices of
 * sym_blocks(Kmax) blocks of 64 x 64 each in the layout above with kb = ceil(nf[b] / 64) block rows, holding the LOWER blocks of a
 * symmetric positive definite matrix of order nf[b] (nf: B int32 on the device) padded with the identity to 64 kb, float32.  One
 * workgroup per problem runs what k_bwd_chol_solve would for that block count (f16 = 1: its float16 tile products) and leaves L_ij
 * below the diagonal, inv(L_jj) on it.  which = 0: every pivot block eliminates its 64 columns, 1: the last one stops behind
 * column nf[b] (what LQP_PIV_COLS=1 runs).  info_out: B int32, 0 or 1 + the index of the first pivot that is not positive.
 * Kmax <= 8.  No reference counterpart. */
int lqp_debug_chol_factor(void* stream, int B, int Kmax, void* packed_inout, const void* nf, int f16, int which, void* info_out);

/* ---- forward ADMM solve ------------------------------------------------
 * Replaces torch_solve_box_qp (lqp_py/solve_box_qp_admm_torch.py:108-333):
 * scaling :160-197, rho :199-203, KKT assembly + LU :205-215, the hot loop
 * :235-313 (lu_solve :267, clamp :271-276, residuals :279-282, check
 * :285-313, adaptive-rho refactor :237-256) and unscale/duals :315-327.
 * Shapes: Q (B,n,n) p (B,n,1) A (B,m,n)|NULL b (B,m,1)|NULL lb,ub (B,n,1);
 * outputs x,z,u (B,n,1) lams (B,2n,1) nus (B,m,1)|NULL rho_out (B) (always
 * written, one value per problem).  rho_in: B values when rho_mode == 2.  */
size_t lqp_boxqp_forward_workspace_bytes(int dtype, int B, int n, int m);
/* Where, inside the workspace, the device-side status block (16 int32: [0] done, [1] final iteration,
 * [3] adaptive-rho refactorisations, [4] rho updated, [5] grid-barrier timeout, [7] linsolve 2 met a matrix
 * that is not positive definite: results invalid, repeat with linsolve 1, [12] / [13] some lower / upper bound of the
 * batch is finite) and the per-problem LU
 * info array (B int32, non-zero = exactly singular) live -- for callers that skipped the host sync
 * (ctrl.reserved = 1) and fetch them asynchronously. */
int lqp_boxqp_forward_layout(int dtype, int B, int n, int m, size_t* status_offset, size_t* status_bytes,
                             size_t* info_offset, size_t* info_bytes);
int lqp_boxqp_forward(void* stream, int dtype, int B, int n, int m,
                      const void* Q, const void* p, const void* A, const void* b,
                      const void* lb, const void* ub,
                      const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                      void* x, void* z, void* u, void* lams, void* nus, void* rho_out,
                      lqp_boxqp_stats* stats,
                      void* workspace, size_t workspace_bytes);

/* Second half of a split synchronous forward (ctrl.reserved = 2, stats.mode_used == 4 on return): waits until the
 * forward's last kernel has stored its report into `host_report` -- the pinned words are POLLED, the stream is not
 * synchronised: the outputs are stream-ordered like those of any asynchronous operator -- and completes `stats`
 * (the same struct the forward call filled).  max_iters / check_solved: the values of the ctrl struct of that call.
 * Returns what the synchronous call would have: LQP_OK, LQP_ERR_SINGULAR (stats.fail_index), LQP_ERR_TIMEOUT, or
 * LQP_ERR_NOT_SPD: repeat the forward with ctrl.linsolve = 1 (a one-call synchronous forward does that by itself). */
int lqp_boxqp_forward_finish(void* stream, int B, int max_iters, int check_solved, const void* host_report,
                             lqp_boxqp_stats* stats);

/* ---- unroll=True: backward through the unrolled ADMM loop ------------------------------------------------
 * The reference's `unroll` mode (lqp_py/solve_box_qp_admm_torch.py:14-15, 216-219, 255-256, 264-265) lets autograd tape
 * every iteration, each x-update being TorchLULayer (lqp_py/lu_layer.py:25-58: backward dx = lu_solve(LU, P, -g),
 * dA = dx x^T, db = -dx).  With a constant factor that tape is ONE reverse recurrence: this entry replays the `iters + 1`
 * x-updates of the float32 forward that used `fwd_workspace` (it must have run the symmetric x-update WITHOUT an
 * adaptive-rho refactorisation, with ctrl.reserved2 bit 0 set so that its factor is complete in the workspace; nothing
 * else may have used that workspace since) and walks back through them.  Outputs are the gradients w.r.t. the SCALED
 * problem the loop ran on -- dQs (B,n,n; NULL = skip), dps (B,n), dAs (B,m,n), dbs (B,m), dlbs, dubs (B,n), drho (B) --
 * and dD (B,n) = dl_dx * x_scaled (the returned x is D x); the caller chains them through the scaling (:160-203).
 * dl_dx (B,n): gradient w.r.t. the returned solution.  float32 only.                                            */
size_t lqp_boxqp_unroll_backward_workspace_bytes(int B, int n, int m, int iters);
int lqp_boxqp_unroll_backward(void* stream, int B, int n, int m, const void* fwd_workspace, size_t fwd_workspace_bytes,
                              int iters, const void* dl_dx, void* dQs, void* dps, void* dAs, void* dbs, void* dlbs,
                              void* dubs, void* drho, void* dD, void* scratch, size_t scratch_bytes);

/* ABI 13: the same reverse recurrence for a forward that ran the PIVOTED LU of the KKT matrix (stats.linsolve_used == 1: float64,
 * more than 16 equality rows, a non-symmetric Q, ctrl.linsolve = 1) without a refactorisation -- the tape's node is
 * TorchLULayer as it stands (lqp_py/lu_layer.py:25-58: forward lu_solve with the cached factor, backward dxv = lu_solve(LU, P, -g)
 * with the SAME factor, dM = dxv xv^T, drhs = -dxv; xv = [x; nu]): `iters + 1` cached solves to replay the loop, as many to walk it
 * back, on the packed factor the forward left in `fwd_workspace`.  Same outputs as lqp_boxqp_unroll_backward, in `dtype`;
 * n + m up to what the forward takes.  Replaces the eager tape of lqp_py/solve_box_qp_admm_torch.py:235-313 under unroll=True. */
size_t lqp_boxqp_unroll_backward_lu_workspace_bytes(int dtype, int B, int n, int m, int iters);
int lqp_boxqp_unroll_backward_lu(void* stream, int dtype, int B, int n, int m, const void* fwd_workspace, size_t fwd_workspace_bytes,
                                 int iters, const void* dl_dx, void* dQs, void* dps, void* dAs, void* dbs, void* dlbs, void* dubs,
                                 void* drho, void* dD, void* scratch, size_t scratch_bytes);

/* ABI 13: a tape whose factor CHANGES along it -- a solve in which rho was adapted (solve_box_qp_admm_torch.py:237-256 inside the
 * tape).  The caller walks it epoch by epoch: for every epoch the packed factor of ITS KKT matrix (`packed_buf`: what lqp_lu_pack
 * filled; NULL: the forward's) and its rho (B values; NULL: the forward's), the x-updates [k0, k1) of the `iters + 1` recorded ones.
 * mode bit 0: replay them from `state` = (z, u) (B,2,n; read when k0 > 0, written when k1 < iters + 1) into the scratch rows;
 * mode bit 1: walk them back -- `state` = the cotangents of (z, u) at k1 (read when k1 < iters + 1, written when k0 > 0), dps /
 * dlbs / dubs accumulate over the segments, drho is THIS segment's, dD is written by the last one (k1 == iters + 1); `inj` (B,4,n):
 * cotangents the caller adds at x-update `inj_k` to x_c | z_{c+1} | u_{c+1} | z_c -- what the gradient of the NEXT epoch's rho sends
 * into the iterates of the check it was computed from.  z_rows / u_rows / x_rows (may be NULL): where the scratch keeps
 * z_{k+1}, u_{k+1}, x_k as (B, iters + 1, n) (k1 <= k0: only this query).  lqp_boxqp_unroll_tape_finish: dQs, dAs, dbs over the whole
 * tape once every segment has been walked.  The tape's nodes are TorchLULayer's (lu_layer.py:25-58), as in
 * lqp_boxqp_unroll_backward_lu. */
size_t lqp_boxqp_unroll_tape_workspace_bytes(int dtype, int B, int n, int m, int iters);
int lqp_boxqp_unroll_tape_segment(void* stream, int dtype, int B, int n, int m, const void* fwd_workspace, size_t fwd_workspace_bytes,
                                  int iters, int k0, int k1, int mode, const void* packed_buf, const void* rho, void* state, int inj_k,
                                  const void* inj, const void* dl_dx, void* dps, void* dlbs, void* dubs, void* drho, void* dD,
                                  void* scratch, size_t scratch_bytes, void** z_rows, void** u_rows, void** x_rows);
int lqp_boxqp_unroll_tape_finish(void* stream, int dtype, int B, int n, int m, int iters, void* dQs, void* dAs, void* dbs, void* scratch,
                                 size_t scratch_bytes);

/* The scaling (solve_box_qp_admm_torch.py:160-203) behind the unrolled loop (ABI 10): what of its derivative walks over the
 * (B,n,n) tensors, one pass each; the reference lets autograd tape these as torch ops (:163 column maxima of |Q| --
 * torch.linalg.norm(ord=inf, dim=1) --, :176 Qs = D Q D, :201 ||Qs||_F and their backward nodes: ~25 passes over Q-sized
 * tensors), and the n-sized rest of the chain (quantiles / beta :169-175, equality rows :179-190, bounds :192-194) in one
 * kernel.  float32; Q (B,n,n) row-major; d (B,n) the scaling vector or NULL (scale = False).
 *   colmax   colmax_j = max_i |Q_ij| (B,n) float, argmax (B,n) int32 = the first row attaining it, count (B,n) int32 = how many do
 *   grad     G (B,n,n) in: dL/dQs (lqp_boxqp_unroll_backward's dQs); out: D (G + s D Q D) D with s (B) = dL/d||Qs||_F / ||Qs||_F
 *            (||Qs||_F = rho sqrt(n) of the forward where :201-203 did not clamp, else the term is zero) or NULL = 0;
 *            parts (B, 1 + slabs, n): [0] r_i = sum_j T_ij Q_ij d_j, [1 + y] the share of row slab y in c_j = sum_i T_ij d_i Q_ij,
 *            T = G + s D Q D: dL/dd through Qs is parts.sum(1); slabs = lqp_unroll_scale_grad_slabs(B, n)
 *   scatter  G_ij += g_colmax_j sign(Q_ij) / count_j wherever |Q_ij| = colmax_j (amax shares its gradient between ties)   */
int lqp_unroll_scale_colmax(void* stream, int B, int n, const void* Q, void* colmax, void* argmax, void* count);
int lqp_unroll_scale_grad_slabs(int B, int n);
int lqp_unroll_scale_grad(void* stream, int B, int n, const void* Q, const void* d, const void* s, void* G, void* parts, int slabs);
/*   vectors  the n-sized rest of the chain for scale = True, one workgroup per problem.  phase 0: d_out (B,n) = the scaling vector from
 *            colmax (floor :164-168, d0 = colmax^-1/2, beta = 1 - q10(d0) / q90(d0) with torch.quantile's interpolation unless
 *            beta_given, d = (1 - beta) d0 + beta mean(d0), :169-175).  phase 1: its backward and that of ps = d p, As = E (A d),
 *            bs = E b (E = 1 / row maxima of |A d|, floored, :179-190), lbs = lb / d, ubs = ub / d (has_box, :192-194): from the
 *            upstream gradients g_ps (B,n), g_As (B,m,n), g_bs (B,m), g_lbs, g_ubs, g_D (B,n) (any may be NULL = 0) and `parts`
 *            (B,nparts,n; summed over nparts: dL/dd through Qs, from `grad`) to dp, dA, db, dlb, dub (NULL = skip) and g_colmax (B,n),
 *            node by node as autograd takes it (amax shares its gradient between ties, the quantile passes it to its two
 *            neighbours); an infinite bound contributes nothing (0 * inf taken as 0).  n <= ~8000 (LDS), float32.            */
int lqp_unroll_scale_vectors(void* stream, int B, int n, int m, int phase, int has_box, int beta_given, double beta_value,
                             const void* colmax, const void* p, const void* A, const void* b, const void* lb, const void* ub,
                             const void* g_ps, const void* g_As, const void* g_bs, const void* g_lbs, const void* g_ubs, const void* g_D,
                             const void* parts, int nparts, void* d_out, void* dp, void* dA, void* db, void* dlb, void* dub,
                             void* g_colmax);
int lqp_unroll_scale_scatter(void* stream, int B, int n, const void* Q, const void* colmax, const void* argmax, const void* count,
                             const void* g_colmax, void* G);

/* Primal / dual error (inf-norms of D r and D s, :287-288) of the LAST convergence check of the forward that
 * used `workspace`, one value per problem -- the two numbers the reference's NumPy solver returns next to the
 * solution (lqp_py/solve_box_qp_admm.py:265-267).  Either output may be NULL.                              */
int lqp_boxqp_last_residuals(void* stream, int dtype, int B, int n, int m,
                             const void* workspace, size_t workspace_bytes,
                             void* primal_out, void* dual_out);

/* ABI 14: the iteration count of every problem of the LAST forward that used `workspace`, which must have run with
 * ctrl.reserved2 bit 3 (LQP_ERR_INVALID otherwise): iters_out[b] = the iteration at whose check problem b was optimal,
 * or max_iters - 1 for one that never was -- B int32 on the DEVICE.  Enqueued on `stream`, nothing is waited for.
 * Which forward ran last on a workspace the library remembers by its ADDRESS until the next forward on that address: a
 * workspace that was freed and whose memory came back as another one is the caller's to keep apart.  After such a forward
 * lqp_boxqp_stats.n_factor counts factorisation launches as always; an event inside the continuation kernel counts once when
 * any problem refactorised at it.                                                                                          */
int lqp_boxqp_problem_iters(void* stream, int dtype, int B, int n, int m,
                            const void* workspace, size_t workspace_bytes, int32_t* iters_out);

/* ---- primal infeasibility detection (added within ABI 17: new symbols only, no struct and no offset changed) ----------
 * lqp_boxqp_forward_detect is lqp_boxqp_forward (the same implementation; lqp_boxqp_forward is the call with detection off)
 * with one more test at every stopping check of a problem: the differences dy, dg, dnu of y = rho u, g = Qs x + s and nu
 * between this check and the last one of the same problem (all in the scaled problem the loop iterates on) give
 *   N = |dy|_inf,  c1 = |dg|_inf / N,  c2 = (sum_i [ubs_i max(dy_i, 0) + lbs_i min(dy_i, 0)] + bs^T dnu) / N
 * and the problem is PRIMAL INFEASIBLE iff N > 0, c1 <= eps_prim_inf and c2 <= -eps_prim_inf (a term of an infinite bound counts
 * 0 while |dy_i| <= eps_prim_inf N and makes c2 = +inf otherwise): OSQP's Farkas certificate of {A x = b, lb <= x <= ub} =
 * empty, with differences taken check to check.  A check behind a change of the problem's rho only refreshes the snapshot.
 * Optimality is tested first.  A flagged problem stops like an optimal one: its iterate of that check is what x, z, u, nus
 * hold, lqp_boxqp_problem_iters names the check, lqp_boxqp_problem_status says 2, and bit 16 of its flag word in
 * ctrl.host_report is set.
 * It needs ctrl.reserved2 bit 3 (every problem stops on its own) and refuses ctrl.check_hook and reserved2 bit 0;
 * eps_prim_inf must be finite and inside (0, 1).  LQP_ERR_INVALID otherwise, before anything is touched.  The workspace is
 * lqp_boxqp_forward_detect_workspace_bytes: the forward's layout, unchanged, and behind it two snapshots (2 n + m values and
 * four words of the solve's dtype each) per problem, which a kernel of the call initialises.  The rho = 0 one-shot (no finite
 * bound in the batch) does not iterate and ignores eps_prim_inf.                                                             */
size_t lqp_boxqp_forward_detect_workspace_bytes(int dtype, int B, int n, int m);
int lqp_boxqp_forward_detect(void* stream, int dtype, int B, int n, int m,
                             const void* Q, const void* p, const void* A, const void* b,
                             const void* lb, const void* ub,
                             const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                             void* x, void* z, void* u, void* lams, void* nus, void* rho_out,
                             lqp_boxqp_stats* stats,
                             void* workspace, size_t workspace_bytes, double eps_prim_inf);
/* ---- dual infeasibility detection (added within ABI 17: new symbols only, no struct and no signature changed) ----------
 * lqp_boxqp_forward_certify is the same implementation once more (lqp_boxqp_forward_detect is the call with eps_dual_inf = 0)
 * with a second test at every stopping check of a problem, on the same snapshot: with dx, dq the differences of x and Qs x
 * (scaled problem; Qs x is formed from the x-update's right-hand side, Q is not read) between this check and the last one,
 *   N = |dx|_inf,  e1 = |dq|_inf / N,  e2 = ps^T dx / N,  e3 = max_i([lbs_i finite] (-dx_i), [ubs_i finite] dx_i, 0) / N
 * and the problem is DUAL INFEASIBLE -- its objective is unbounded below on its feasible set -- iff N > 0, e1 <= eps_dual_inf,
 * e2 <= -eps_dual_inf and e3 <= eps_dual_inf: OSQP's certificate with differences taken check to check, except that As dx is
 * not tested (the x-update solves the equality-constrained system: As x = bs holds at every iteration to rounding).  Order in a
 * check: optimal, primal infeasible, dual infeasible.  A flagged problem stops like an optimal one with the iterate of that
 * check; lqp_boxqp_problem_status says 3 and bit 17 of its flag word in ctrl.host_report is set.
 * Either threshold is 0 (that certificate is off) or finite and inside (0, 1), and at least one is not 0; the other refusals
 * are lqp_boxqp_forward_detect's (reserved2 bit 3 required, no check_hook, no bit 0): LQP_ERR_INVALID before anything is
 * touched.  lqp_boxqp_forward_certify_workspace_bytes is the size with both certificates on: the forward's layout, unchanged,
 * and behind it two snapshots of 4 n + m values and four words each per problem (with eps_dual_inf = 0 the size and the layout
 * of lqp_boxqp_forward_detect are enough, and are what is used).  The rho = 0 one-shot ignores both thresholds.              */
size_t lqp_boxqp_forward_certify_workspace_bytes(int dtype, int B, int n, int m);
int lqp_boxqp_forward_certify(void* stream, int dtype, int B, int n, int m,
                              const void* Q, const void* p, const void* A, const void* b,
                              const void* lb, const void* ub,
                              const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                              void* x, void* z, void* u, void* lams, void* nus, void* rho_out,
                              lqp_boxqp_stats* stats,
                              void* workspace, size_t workspace_bytes, double eps_prim_inf, double eps_dual_inf);
/* ---- an L1 term in the objective (added within ABI 17: new symbols only, no struct and no signature changed) ---------------
 *   min 0.5 x'Qx + p'x + sum_i w_i |x_i - c_i|   s.t.  A x = b,  lb <= x <= ub,     w >= 0 and c finite, (B,n,1) like p
 * (turnover / transaction cost around yesterday's holdings c).  lqp_boxqp_forward_l1 is the same implementation once more with
 * another z-update: in the scaled space of the loop (x = D xs) the data are ws = D w, cs = c / D, and with v = xh + u (xh as in
 * lqp_boxqp_forward, over-relaxation included), t = ws / rho (the rho of this iteration) and d = v - cs
 *   S = v - t if d > t,  v + t if d < -t,  cs otherwise;     z = min(max(S, lbs), ubs)
 * -- soft-threshold around cs, then clamp.  x-update, factorisations, stopping rule, rho adaptation: unchanged; w = 0 gives
 * lqp_boxqp_forward's x, z, u bit for bit.  The solve always iterates: bounds that are all infinite are an ordinary case, the
 * rho = 0 one-shot does not exist here (rho_mode 1 with rho_value <= 0: LQP_ERR_INVALID), ctrl.any_lb / any_ub are not read.
 * Every loop kernel family has instances with this step (the small loop, the split loop on two and four workgroups, the
 * streaming loop on one and two) except the dense LU tiers, whose problems run the streaming loop's LU branch.
 * Two more outputs, (B,n,1) in the solve's dtype, from the step evaluated once more at the returned iterate (v = zs + us, in the
 * scaled space, where an element on the kink has zs == cs exactly):
 *   side   sign(S - cs): +1 / -1 off the kink, 0 exactly on the kink set K (the "otherwise" branch with t > 0)
 *   u_box  (S - clamp(S)) / D -- S - zs with the clamp taken again at this v, so exactly zero unless the element is clamped:
 *          the box's share of the dual u; lams is built from IT here, lams = [relu(-rho u_box); relu(rho u_box)] -- the
 *          rest of u is the L1 term's multiplier.
 * Refused with LQP_ERR_INVALID before anything is touched: a null w, c, side or u_box, ctrl.reserved2 bit 3 (per-problem
 * stopping) or bit 0 (the factor kept for the unroll sweep), a check_hook.  A weight that is negative or not finite, and a
 * rho of a problem (rho_mode 2: an entry of rho_in) that is not positive and finite, is found
 * on the device: the problem's outputs are NaN, bit 18 (262144) of its flag word in ctrl.host_report is set, and a call that
 * waits returns LQP_ERR_INVALID with stats.fail_index naming it.  lqp_boxqp_forward_l1_workspace_bytes: the forward's layout,
 * unchanged, and behind it 3 n values per problem (ws, cs, t), written by a kernel of the call before any loop kernel runs.   */
size_t lqp_boxqp_forward_l1_workspace_bytes(int dtype, int B, int n, int m);
int lqp_boxqp_forward_l1(void* stream, int dtype, int B, int n, int m,
                         const void* Q, const void* p, const void* A, const void* b,
                         const void* lb, const void* ub, const void* w, const void* c,
                         const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                         void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* side, void* u_box,
                         lqp_boxqp_stats* stats,
                         void* workspace, size_t workspace_bytes);
/* Its backward needs no factorisation of its own: an element on the kink behaves like one whose two bounds are both c_i, a
 * thresholded free element like p_i shifted by side_i w_i.  Two element-wise kernels around lqp_boxqp_backward_fp, which runs
 * unchanged on (dl_dz, x, u_e, lams_e, nus, Q, A, lb_e, ub_e, rho):
 *   lqp_boxqp_l1_effective_box   K = (side == 0):  lb_e = K ? c : lb,  ub_e = K ? c : ub,  u_e = K ? u : u_box,
 *                                lams_e = [relu(-rho u_e); relu(rho u_e)] (B,2n,1); rho_mode 1 = rho_value, 2 = rho_in (B)
 *   lqp_boxqp_l1_finish_grads    dlb = K ? 0 : dlb_e,  dub = K ? 0 : dub_e,  dc = K ? dlb_e + dub_e : 0,  dw = side * dp;
 *                                any of dlb, dub, dc, dw may be NULL = skip, dlb / dub may be dlb_e / dub_e themselves.
 * dQ, dp, dA, db are lqp_boxqp_backward_fp's.  All (B,n,1) in `dtype`; enqueued on `stream`, nothing is waited for.          */
int lqp_boxqp_l1_effective_box(void* stream, int dtype, int B, int n,
                               const void* side, const void* u, const void* u_box,
                               const void* lb, const void* ub, const void* c,
                               int rho_mode, double rho_value, const void* rho_in,
                               void* lb_e, void* ub_e, void* u_e, void* lams_e);
int lqp_boxqp_l1_finish_grads(void* stream, int dtype, int B, int n,
                              const void* side, const void* dp, const void* dlb_e, const void* dub_e,
                              void* dlb, void* dub, void* dc, void* dw);
/* ---- a soft band in the objective (added within ABI 17: new symbols only, no struct and no signature changed) --------------
 *   min 0.5 x'Qx + p'x + sum_i [ wl_i (lo_i - x_i)_+ + wu_i (x_i - hi_i)_+ ]   s.t.  A x = b,  lb <= x <= ub
 *   wl, wu >= 0 and finite;  lo <= hi, lo finite or -inf, hi finite or +inf;  all four (B,n,1) like p
 * (soft position limits inside the hard box, a no-cost band, a one-sided hinge, asymmetric costs; lo = hi = c with wl = wu = w is
 * the L1 term).  lqp_boxqp_forward_soft is the same implementation once more with another z-update: in the scaled space of the
 * loop the data are wls = D wl, wus = D wu, los = lo / D, his = hi / D, and with v = xh + u (xh as in lqp_boxqp_forward,
 * over-relaxation included), tl = wls / rho, tu = wus / rho (the rho of this iteration), dh = v - his, dl = v - los
 *   S = v - tu if dh > tu,  v + tl if dl < -tl,  min(max(v, los), his) otherwise;     z = min(max(S, lbs), ubs)
 * x-update, factorisations, stopping rule, rho adaptation: unchanged; wl = wu = 0 gives lqp_boxqp_forward's x, z, u bit for bit,
 * lo = hi with wl = wu gives lqp_boxqp_forward_l1's.  The solve always iterates: bounds that are all infinite are an ordinary
 * case, the rho = 0 one-shot does not exist here (rho_mode 1 with rho_value <= 0: LQP_ERR_INVALID), ctrl.any_lb / any_ub are not
 * read.  The same loop kernel families as the L1 term have instances with this step; the dense LU tiers' problems run the
 * streaming loop's LU branch.
 * Two more outputs, (B,n,1) in the solve's dtype, from the step evaluated once more at the returned iterate (v = zs + us):
 *   zone   +2 if dh > tu, -2 if dl < -tl, else +1 if v >= his and tu > 0, else -1 if v <= los and tl > 0, else 0 -- the sloped
 *          pieces, the kinks hi / lo (zs == his / los exactly there), the inside of the band
 *   u_box  (S - clamp(S)) / D, exactly zero unless the element is clamped: the box's share of the dual u; lams is built from
 *          it, lams = [relu(-rho u_box); relu(rho u_box)] -- the rest of u is the band's multiplier, in [-wl, wu] / rho.
 * Refused with LQP_ERR_INVALID before anything is touched: a null wl, wu, lo, hi, zone or u_box, ctrl.reserved2 bit 3
 * (per-problem stopping) or bit 0 (the factor kept for the unroll sweep), a check_hook.  A weight that is negative or not finite,
 * lo > hi, a NaN in lo or hi, and a rho of a problem (rho_mode 2: an entry of rho_in) that is not positive and finite, is found on
 * the device: the problem's outputs are NaN, bit 19 (524288) of its flag word in ctrl.host_report is set, and a call that waits
 * returns LQP_ERR_INVALID with stats.fail_index naming it.  lqp_boxqp_forward_soft_workspace_bytes: the forward's layout,
 * unchanged, and behind it 6 n values per problem (wls, wus, los, his, tl, tu), written by kernels of the call before they are read. */
size_t lqp_boxqp_forward_soft_workspace_bytes(int dtype, int B, int n, int m);
int lqp_boxqp_forward_soft(void* stream, int dtype, int B, int n, int m,
                           const void* Q, const void* p, const void* A, const void* b,
                           const void* lb, const void* ub, const void* wl, const void* wu, const void* lo, const void* hi,
                           const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                           void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* zone, void* u_box,
                           lqp_boxqp_stats* stats,
                           void* workspace, size_t workspace_bytes);
/* Its backward: an element on a kink behaves like one whose two bounds are both that kink, a free element on a sloped piece like
 * p_i shifted by wu_i / -wl_i.  A kink that lies beyond a hard bound holds nothing -- the bound does (u_box != 0), and the element
 * is an ordinary clamped one.  Two element-wise kernels around lqp_boxqp_backward_fp, which runs unchanged on
 * (dl_dz, x, u_e, lams_e, nus, Q, A, lb_e, ub_e, rho):
 *   lqp_boxqp_soft_effective_box   Kl = (zone == -1 and u_box == 0), Kh = (zone == +1 and u_box == 0), K = Kl or Kh, kv = Kh ? hi : lo:
 *                                  lb_e = K ? kv : lb,  ub_e = K ? kv : ub,  u_e = K ? u : u_box,
 *                                  lams_e = [relu(-rho u_e); relu(rho u_e)] (B,2n,1); rho_mode 1 = rho_value, 2 = rho_in (B)
 *   lqp_boxqp_soft_finish_grads    dlb = K ? 0 : dlb_e,  dub = K ? 0 : dub_e,  dlo = Kl ? dlb_e + dub_e : 0,  dhi = Kh ? dlb_e + dub_e : 0,
 *                                  dwu = (zone == +2) ? dp : 0,  dwl = (zone == -2) ? -dp : 0; any of the six outputs may be NULL =
 *                                  skip, dlb / dub may be dlb_e / dub_e themselves.
 * dQ, dp, dA, db are lqp_boxqp_backward_fp's.  All (B,n,1) in `dtype`; enqueued on `stream`, nothing is waited for.          */
int lqp_boxqp_soft_effective_box(void* stream, int dtype, int B, int n,
                                 const void* zone, const void* u, const void* u_box,
                                 const void* lb, const void* ub, const void* lo, const void* hi,
                                 int rho_mode, double rho_value, const void* rho_in,
                                 void* lb_e, void* ub_e, void* u_e, void* lams_e);
int lqp_boxqp_soft_finish_grads(void* stream, int dtype, int B, int n,
                                const void* zone, const void* u_box, const void* dp, const void* dlb_e, const void* dub_e,
                                void* dlb, void* dub, void* dwl, void* dwu, void* dlo, void* dhi);
/* ---- a log barrier in the objective (added within ABI 17: new symbols only, no struct and no signature changed) -------------
 *   min 0.5 x'Qx + p'x - sum_i w_i log(x_i)   s.t.  A x = b,  lb <= x <= ub;     w >= 0 and finite, (B,n,1) like p
 * (risk budgeting: Q = Sigma, w the budgets; a long-only barrier that keeps holdings off zero; Kelly / log-utility terms).
 * lqp_boxqp_forward_log is the same implementation once more with another z-update.  In the scaled space of the loop
 * (x = D xs) the term is -w_i log(xs_i) plus a constant, so the weight takes no D: ws = w; only the equality rows carry E,
 * the objective has no scalar scale.  With v = xh + u (xh as in lqp_boxqp_forward, over-relaxation included), t = ws / rho
 * (the rho of this iteration, a true division) and s = sqrt(v v + 4 t):
 *   S = v              if t == 0     (a branch: w = 0 returns lqp_boxqp_forward's x, z, u bit for bit)
 *   S = 0.5 (v + s)    if v >= 0
 *   S = 2 t / (s - v)  if v <  0     (the form without cancellation)
 *   z = min(max(S, lbs), ubs)
 * x-update, factorisations, stopping rule, rho adaptation: unchanged.  The solve always iterates: bounds that are all
 * infinite are an ordinary case, the rho = 0 one-shot does not exist here (rho_mode 1 with rho_value <= 0:
 * LQP_ERR_INVALID), ctrl.any_lb / any_ub are not read.  The same loop kernel families as the L1 term and the soft band have
 * instances with this step; the dense LU tiers' problems run the streaming loop's LU branch.
 * Two more outputs, (B,n,1) in the solve's dtype, from the step evaluated once more at the returned iterate (v = zs + us):
 *   u_box  the box's share of the dual u: (us + t / zs) / D, i.e. rho u + w / z unscaled and divided by rho, on an element
 *          where S != clamp(S); exactly zero everywhere else.  (S - zs) / D is NOT the bound's multiplier here: the barrier
 *          pushes on a clamped element too.  lams = [relu(-rho u_box); relu(rho u_box)].
 *   curv   w_i / z_i^2 (the unscaled z) where w_i > 0 and u_box_i == 0, else 0: the diagonal of the term's Hessian on the
 *          free set, for lqp_boxqp_backward_fp_curv.
 * Refused with LQP_ERR_INVALID before anything is touched: a null w, u_box or curv, ctrl.reserved2 bit 3 (per-problem
 * stopping) or bit 0 (the factor kept for the unroll sweep), a check_hook.  A weight that is negative or not finite, w_i > 0
 * with ub_i <= 0 (the domain is empty), and a rho of a problem (rho_mode 2: an entry of rho_in) that is not positive and
 * finite, is found on the device: the problem's outputs are NaN, bit 20 (1048576) of its flag word in ctrl.host_report is
 * set, and a call that waits returns LQP_ERR_INVALID with stats.fail_index naming it.
 * lqp_boxqp_forward_log_workspace_bytes: the forward's layout, unchanged, and behind it 2 n values per problem (ws, t),
 * written by kernels of the call before they are read. */
size_t lqp_boxqp_forward_log_workspace_bytes(int dtype, int B, int n, int m);
int lqp_boxqp_forward_log(void* stream, int dtype, int B, int n, int m,
                          const void* Q, const void* p, const void* A, const void* b,
                          const void* lb, const void* ub, const void* w,
                          const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                          void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* u_box, void* curv,
                          lqp_boxqp_stats* stats,
                          void* workspace, size_t workspace_bytes);
/* lqp_boxqp_backward_fp with a caller's diagonal: curv (B,n,1), non-negative, or NULL.  The free-set system becomes
 * [[Q_FF + diag(curv_F), A_F^T], [A_F, 0]] (+1e-8 I): curv_i joins the 1e-8 of free variable i in every build (the full
 * system, the reduced one, the Cholesky form with its equilibration scale) and in the residual of the LU form's refinement
 * step; entries of clamped variables are not read into the system (their dx is 0).  It is the hook for a smooth separable
 * term of the objective: the term supplies its prox in the forward and its second derivative here.  NULL or all-zero curv
 * returns lqp_boxqp_backward_fp's results bit for bit.  There is no prefactor phase with a diagonal: linsolve with
 * LQP_BWD_PREFACTORED is refused with LQP_ERR_INVALID.  Workspace: lqp_boxqp_backward_fp_workspace_bytes. */
int lqp_boxqp_backward_fp_curv(void* stream, int dtype, int B, int n, int m,
                               const void* dl_dz, const void* x, const void* u, const void* lams, const void* nus,
                               const void* Q, const void* A, const void* lb, const void* ub, const void* curv,
                               int rho_mode, double rho_value, const void* rho_in,
                               void* dQ, void* dp, void* dA, void* db, void* dlb, void* dub,
                               int32_t* fail_index, void* workspace, size_t workspace_bytes, int linsolve, void* host_report);
/* The backward of lqp_boxqp_forward_log: lqp_boxqp_backward_fp_curv on (dl_dz, x, u_e, lams_e, nus, Q, A, lb, ub, curv, rho)
 * with the true lb, ub, between two element-wise kernels:
 *   lqp_boxqp_log_effective_duals  u_e = u_box,  lams_e = [relu(-rho u_e); relu(rho u_e)] (B,2n,1); rho_mode 1 = rho_value,
 *                                  2 = rho_in (B)
 *   lqp_boxqp_log_finish_grads     dw_i = -dp_i / z_i where w_i > 0, else 0 (the convention at w_i = 0: the one-sided
 *                                  derivative is not defined there when x_i <= 0); dw may be NULL = nothing is done.
 * dQ, dp, dA, db, dlb, dub are the backward's own (a clamped element has dx_i = 0: curv never enters its row).
 * All (B,n,1) in `dtype`; enqueued on `stream`, nothing is waited for. */
int lqp_boxqp_log_effective_duals(void* stream, int dtype, int B, int n, const void* u_box,
                                  int rho_mode, double rho_value, const void* rho_in, void* u_e, void* lams_e);
int lqp_boxqp_log_finish_grads(void* stream, int dtype, int B, int n, const void* dp, const void* z, const void* w, void* dw);
/* ---- a piecewise-linear term in the objective (added within ABI 17: new symbols only, no struct and no signature changed) ---
 *   min 0.5 x'Qx + p'x + sum_i f_i(x_i)   s.t.  A x = b,  lb <= x <= ub
 *   f_i(x) = s_i0 x + sum_{k=1..K} (s_ik - s_i,k-1) (x - c_ik)_+ ,   1 <= K <= 3
 *   slopes s_i0 <= ... <= s_iK, finite;  kinks c_i1 <= ... <= c_iK, no NaN, -inf allowed at the low end and +inf at the high end
 * (convex, K kinks, K + 1 slopes per element: the L1 term is K = 1 with slopes -w, w; the soft band K = 2 with slopes -wl, 0, wu; both
 * at once, two-tier trading costs c - delta, c, c + delta, asymmetric buy and sell tiers are K = 3.)
 * Layout: s is [K + 1][B][n] and c is [K][B][n] -- slope k / kink k of every element as one (B,n,1) vector, the vectors one
 * behind the other.  The kernels are written for three kinks; K < 3 is padded at the top by this entry (a kink at +inf, the last
 * slope once more), which does not change any piece number.
 * lqp_boxqp_forward_pwl is the same implementation once more with another z-update: in the scaled space of the loop the data are
 * ss_k = D s_k, cs_k = c_k / D, and with v = xh + u (xh as in lqp_boxqp_forward, over-relaxation included), t_k = ss_k / rho (the
 * rho of this iteration, a true division):
 *   S = v                                   if every slope is zero (a branch: lqp_boxqp_forward's x, z, u bit for bit)
 *   for k = K .. 1:  d = v - cs_k;  S = v - t_k if d > t_k;  S = cs_k if d >= t_{k-1}
 *   S = v - t_0                             otherwise;                                  z = min(max(S, lbs), ubs)
 * -- these comparisons, from the top: slopes (-w, w) give lqp_boxqp_forward_l1's results and (-wl, 0, wu) lqp_boxqp_forward_soft's,
 * bit for bit.  x-update, factorisations, stopping rule, rho adaptation: unchanged.  The solve always iterates: bounds that are
 * all infinite are an ordinary case, the rho = 0 one-shot does not exist here (rho_mode 1 with rho_value <= 0: LQP_ERR_INVALID),
 * ctrl.any_lb / any_ub are not read.  The same loop kernel families as the other terms have instances with this step.
 * Two more outputs, (B,n,1) in the solve's dtype, from the scan taken once more at the returned iterate (v = zs + us):
 *   piece  2 k where the element rests on the slope s_k (d > t_k at kink k, or below every kink: 0), 2 k - 1 exactly on kink k
 *          (zs == cs_k there) -- only where the kink's jump s_k - s_{k-1} is positive; with none the element belongs to the piece
 *          below, 2 k - 2
 *   u_box  (S - clamp(S)) / D, exactly zero unless the element is clamped: the box's share of the dual u; lams is built from it.
 * Refused with LQP_ERR_INVALID before anything is touched: a null s, c, piece or u_box, K outside 1 .. 3, ctrl.reserved2 bit 3
 * (per-problem stopping) or bit 0 (the factor kept for the unroll sweep), a check_hook.  A slope that is not finite, slopes or kinks
 * that decrease, a NaN kink, and a rho of a problem (rho_mode 2: an entry of rho_in) that is not positive and finite, is found on the
 * device: the problem's outputs are NaN, bit 21 (2097152) of its flag word in ctrl.host_report is set, and a call that waits returns
 * LQP_ERR_INVALID with stats.fail_index naming it.  lqp_boxqp_forward_pwl_workspace_bytes: the forward's layout, unchanged, and
 * behind it 11 n values per problem (cs_1..3, ss_0..3, t_0..3), written by kernels of the call before they are read. */
size_t lqp_boxqp_forward_pwl_workspace_bytes(int dtype, int B, int n, int m);
int lqp_boxqp_forward_pwl(void* stream, int dtype, int B, int n, int m,
                          const void* Q, const void* p, const void* A, const void* b,
                          const void* lb, const void* ub, const void* s, const void* c, int K,
                          const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                          void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* piece, void* u_box,
                          lqp_boxqp_stats* stats,
                          void* workspace, size_t workspace_bytes);
/* Its backward: an element on kink k behaves like one whose two bounds are both c_k, a free element on a slope like p_i shifted by
 * that slope.  An element a hard bound holds (u_box != 0) is an ordinary clamped one, whatever kink lies there.  Two element-wise
 * kernels around lqp_boxqp_backward_fp, which runs unchanged on (dl_dz, x, u_e, lams_e, nus, Q, A, lb_e, ub_e, rho); c, ds, dc in the
 * caller's K and the layout above:
 *   lqp_boxqp_pwl_effective_box    on = (piece odd and u_box == 0), k = (piece + 1) / 2:
 *                                  lb_e = on ? c_k : lb,  ub_e = on ? c_k : ub,  u_e = on ? u : u_box,
 *                                  lams_e = [relu(-rho u_e); relu(rho u_e)] (B,2n,1); rho_mode 1 = rho_value, 2 = rho_in (B)
 *   lqp_boxqp_pwl_finish_grads     dlb = on ? 0 : dlb_e,  dub = on ? 0 : dub_e,  dc_k = (on and piece == 2 k - 1) ? dlb_e + dub_e : 0,
 *                                  ds_k = (piece == 2 k) ? dp : 0; any of the four outputs may be NULL = skip, dlb / dub may be
 *                                  dlb_e / dub_e themselves.
 * dQ, dp, dA, db are lqp_boxqp_backward_fp's.  Enqueued on `stream`, nothing is waited for. */
int lqp_boxqp_pwl_effective_box(void* stream, int dtype, int B, int n,
                                const void* piece, const void* u, const void* u_box,
                                const void* lb, const void* ub, const void* c, int K,
                                int rho_mode, double rho_value, const void* rho_in,
                                void* lb_e, void* ub_e, void* u_e, void* lams_e);
int lqp_boxqp_pwl_finish_grads(void* stream, int dtype, int B, int n,
                               const void* piece, const void* u_box, const void* dp, const void* dlb_e, const void* dub_e, int K,
                               void* dlb, void* dub, void* ds, void* dc);
/* ---- a Huber term in the objective (added within ABI 17: new symbols only, no struct and no signature changed) --------------
 *   min 0.5 x'Qx + p'x + sum_i w_i H_{delta_i}(x_i - c_i)   s.t.  A x = b,  lb <= x <= ub
 *   H_delta(d) = 0.5 d^2 for |d| <= delta,  delta |d| - 0.5 delta^2 beyond;   w, c, delta (B,n,1) like p
 * (robust tracking / regression: Q = X'X with bounded coefficients, outliers taken linearly; a trade cost that is quadratic for
 * small trades and linear for large ones).  A pure quadratic can be folded into Q and p by the caller; this cannot, because where
 * the curvature acts depends on the solution.  lqp_boxqp_forward_huber is the same implementation once more with another
 * z-update.  In the scaled space of the loop (x = D xs): ws = D^2 w, cs = c / D, ds = delta / D; with v = xh + u (xh as in
 * lqp_boxqp_forward, over-relaxation included), d = v - cs, t = ws / rho (the rho of the launch, a true division) and, once per
 * element and launch, q = t ds, lim = ds + q, sh = t / (1 + t):
 *   S = v           if t == 0     (a branch: w = 0 returns lqp_boxqp_forward's x, z, u bit for bit)
 *   S = v - q       if d >  lim
 *   S = v + q       if d < -lim
 *   S = v - sh d    otherwise
 *   z = min(max(S, lbs), ubs)
 * delta = +inf is allowed (lim = q = +inf: the quadratic branch always, a weighted least-squares term); delta = 0 is no term.
 * x-update, factorisations, stopping rule, rho adaptation: unchanged.  The solve always iterates, as with the other terms: the
 * rho = 0 one-shot does not exist here (rho_mode 1 with rho_value <= 0: LQP_ERR_INVALID), ctrl.any_lb / any_ub are not read.  The
 * same loop kernel families as the other terms have instances with this step; the dense LU tiers' problems run the streaming
 * loop's LU branch.
 * Two more outputs, (B,n,1) in the solve's dtype, from the step's comparisons once more at the returned iterate (v = zs + us):
 *   zone   +1 / -1 on the upper / lower linear piece, 0 on the quadratic zone and wherever w = 0
 *   u_box  the box's share of the dual u: (us - t clip(zs - cs, -ds, ds)) / D on an element where S != clamp(S); exactly zero
 *          everywhere else.  As for the log barrier, (S - zs) / D is NOT the bound's multiplier: the term pushes on a clamped
 *          element too.  lams = [relu(-rho u_box); relu(rho u_box)].
 * Refused with LQP_ERR_INVALID before anything is touched: a null w, c, delta, zone or u_box, ctrl.reserved2 bit 3 (per-problem
 * stopping) or bit 0 (the factor kept for the unroll sweep), a check_hook; a workspace that is too short: LQP_ERR_WORKSPACE.
 * A weight that is negative or not finite, a delta that is negative or NaN, a c that is not finite, and a rho of a problem
 * (rho_mode 2: an entry of rho_in) that is not positive and finite, is found on the device: the problem's outputs are NaN,
 * bit 22 (4194304) of its flag word in ctrl.host_report is set, and a call that waits returns LQP_ERR_INVALID with
 * stats.fail_index naming it.
 * lqp_boxqp_forward_huber_workspace_bytes: the forward's layout, unchanged, and behind it 6 n values per problem (ws, cs, ds,
 * q, lim, sh), written by kernels of the call before they are read. */
size_t lqp_boxqp_forward_huber_workspace_bytes(int dtype, int B, int n, int m);
int lqp_boxqp_forward_huber(void* stream, int dtype, int B, int n, int m,
                            const void* Q, const void* p, const void* A, const void* b,
                            const void* lb, const void* ub, const void* w, const void* c, const void* delta,
                            const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                            void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* zone, void* u_box,
                            lqp_boxqp_stats* stats,
                            void* workspace, size_t workspace_bytes);
/* The backward of lqp_boxqp_forward_huber: the term is C1, so it has no kink sets -- lqp_boxqp_backward_fp_curv on
 * (dl_dz, x, u_e, lams_e, nus, Q, A, lb, ub, curv, rho) with the true lb, ub, between two element-wise kernels:
 *   lqp_boxqp_huber_effective_duals  u_e = u_box,  lams_e = [relu(-rho u_e); relu(rho u_e)] (B,2n,1),  curv = w where
 *                                    zone == 0, w > 0 and u_box == 0, else 0; rho_mode 1 = rho_value, 2 = rho_in (B)
 *   lqp_boxqp_huber_finish_grads     dw = dp clip(z - c, -delta, delta),  dc = -w dp on zone 0, else 0,  ddelta = w zone dp;
 *                                    each of the three may be NULL.
 * dQ, dp, dA, db, dlb, dub are the backward's own.  All (B,n,1) in `dtype`; enqueued on `stream`, nothing is waited for. */
int lqp_boxqp_huber_effective_duals(void* stream, int dtype, int B, int n, const void* u_box, const void* zone, const void* w,
                                    int rho_mode, double rho_value, const void* rho_in, void* u_e, void* lams_e, void* curv);
int lqp_boxqp_huber_finish_grads(void* stream, int dtype, int B, int n, const void* dp, const void* z, const void* zone,
                                 const void* w, const void* c, const void* delta, void* dw, void* dc, void* ddelta);
/* How every problem of the LAST forward on `workspace` ended, which must have run with ctrl.reserved2 bit 3, detection or not
 * (LQP_ERR_INVALID otherwise, as lqp_boxqp_problem_iters): status_out[b] = 0 optimal, 1 it ended at max_iters without being
 * optimal, 2 primal infeasible, 3 dual infeasible (lqp_boxqp_forward_certify) -- B int32 on the DEVICE.  Enqueued on `stream`,
 * nothing is waited for.                                                                                                     */
int lqp_boxqp_problem_status(void* stream, int dtype, int B, int n, int m,
                             const void* workspace, size_t workspace_bytes, int32_t* status_out);

/* ABI 12: the trace of a forward solve that ran with ctrl.reserved2 bit 2 -- for check c = 0 .. n_checks - 1 (held at
 * iteration c * check_solved) trace_out[2 c] = max over the batch of ||D r||_inf, trace_out[2 c + 1] = max of ||D s||_inf,
 * float32 on the DEVICE (2 * n_checks values; at most 2048 checks are kept).  Replaces the prints of
 * solve_box_qp_admm_torch.py:289-294 (verbose=True): the loop runs on the device without the host, so the lines are
 * printed after the solve from this trace.  Enqueued on `stream`.                                                        */
int lqp_boxqp_check_trace(void* stream, int dtype, int B, int n, int m,
                          const void* workspace, size_t workspace_bytes, int n_checks, void* trace_out);

/* ---- fixed-point implicit backward --------------------------------------
 * Replaces torch_solve_box_qp_grad (solve_box_qp_admm_torch.py:349-432):
 * active-set mask :360-365, non-symmetric system :378-392, linalg.solve
 * :393, gradient epilogue :396-430.  rho_mode 1 = scalar rho_value, 2 =
 * per-problem rho_in.  Any of dQ (B,n,n), dp (B,n,1), dA (B,m,n), db (B,m,1),
 * dlb, dub (B,n,1) may be NULL = skip.  fail_index NULL = do not wait for the
 * GPU (errors stay in the workspace's info array).  linsolve: 0/1 pivoted LU of
 * the system like torch.linalg.solve (:393); 2 = Q is known to be symmetric
 * (the forward ran linsolve 2 on it): blocked Cholesky of the free-set block
 * Q_FF + the Schur complement of the equality rows (f32, n <= 512, m <= 16;
 * otherwise, or when Q_FF is not positive definite, LU).                     */
size_t lqp_boxqp_backward_fp_workspace_bytes(int dtype, int B, int n, int m);
/* The part of the Cholesky form that does not need the cotangent -- the free set (:360-365), Q_FF and its factorisation --
 * enqueued ahead of it, e.g. right behind the forward whose x, u it reads (stream order): a caller that waits for its
 * forward (the reference's semantics) then has the factorisation running while its host code travels from `forward` to
 * `backward`.  lqp_boxqp_backward_fp called afterwards on the SAME workspace (nothing else may have used it in between)
 * with linsolve = 2 | LQP_BWD_PREFACTORED only gathers dl_dz, solves and writes the gradients; a factorisation that
 * failed still ends in that call's pivoted-LU retry.  ABI 11: the LU form (float64, linsolve 0 / 1, sizes without a Cholesky
 * form) has the same two phases -- free set, reduced system, pivoted LU and packed factor ahead; gather, solve, refinement and
 * epilogue behind.  LQP_ERR_UNSUPPORTED: this form has no phases (LQP_BWD_FULL builds) -- nothing was enqueued, call
 * lqp_boxqp_backward_fp without the flag.
 * host_report (optional, pinned host memory, B ints; ABI 11): the factorisation is the only step of the Cholesky form that
 * sends a caller to the LU retry, so its info words are final when this call's last kernel ends -- it stores them there
 * (set to -1 by this call before its first launch).  lqp_boxqp_backward_fp given the SAME buffer and
 * linsolve = 2 | LQP_BWD_PREFACTORED | LQP_BWD_REPORTED neither resets nor stores them again: with fail_index it waits for
 * those words only, i.e. it returns as soon as the factorisation is known to have succeeded, while its own solves and the
 * gradient epilogue still run (stream-ordered results, like every other output of this library).  Without the prefactor call
 * lqp_boxqp_backward_fp's Cholesky form reports at the same point: right behind its factorisation.                       */
#define LQP_BWD_PREFACTORED 0x100
#define LQP_BWD_REPORTED 0x200
int lqp_boxqp_backward_fp_prefactor(void* stream, int dtype, int B, int n, int m,
                                    const void* x, const void* u,
                                    const void* Q, const void* A, const void* lb, const void* ub,
                                    void* workspace, size_t workspace_bytes, int linsolve, void* host_report);
int lqp_boxqp_backward_fp(void* stream, int dtype, int B, int n, int m,
                          const void* dl_dz, const void* x, const void* u,
                          const void* lams, const void* nus,
                          const void* Q, const void* A, const void* lb, const void* ub,
                          int rho_mode, double rho_value, const void* rho_in,
                          void* dQ, void* dp, void* dA, void* db, void* dlb, void* dub,
                          int32_t* fail_index,
                          void* workspace, size_t workspace_bytes,
                          int linsolve,
                          void* host_report);   /* NULL, or pinned host memory of B int32: the last kernel stores the
                                                   per-problem info words there (read instead of a copy when
                                                   fail_index is given, left for the caller when it is NULL)    */

/* ---- KKT-system backward (control['backward'] = 'kkt') -------------------
 * Replaces torch_solve_box_qp_grad_kkt (solve_box_qp_admm_torch.py:435-584) for a batch with finite lower AND upper
 * bounds somewhere (any_lb and any_ub, :439-441).  The reference solves the (3n+m) system
 *     [[Q, G^T diag(lam), A^T], [G, -diag(s), 0], [A, 0, 0]] [dx; dlam; dnu] = [-dl_dz; 0; 0],   G = [-I; I],
 * s = clamp(h - G x, 1e-8), lam = clamp(lams, 1e-8) (:450-452).  Eliminating dlam = diag(1/s) G dx leaves
 *     [[Q + diag(w), A^T], [A, 0]] [dx; dnu] = [-dl_dz; 0],   w = lam_lo / s_lo + lam_hi / s_hi,
 * the same solution on the kernels of the fixed-point backward: every variable free, w in place of its 1e-8
 * regulariser (linsolve 2: blocked Cholesky when Q is known to be symmetric, else pivoted LU), and an epilogue that
 * forms dQ, dp, dA, db (:527-562) and dlb = -dl_dh[:n], dub = dl_dh[n:], dl_dh = -lam dlam (:544, :573-575).
 * Arguments as lqp_boxqp_backward_fp without u / rho.                                                          */
int lqp_boxqp_backward_kkt(void* stream, int dtype, int B, int n, int m, const void* dl_dz, const void* x,
                           const void* lams, const void* nus, const void* Q, const void* A, const void* lb, const void* ub,
                           void* dQ, void* dp, void* dA, void* db, void* dlb, void* dub, int32_t* fail_index,
                           void* workspace, size_t workspace_bytes, int linsolve, void* host_report);

/* ---- batched LU (partial pivoting) and cached LU solve ------------------
 * Replace torch.linalg.lu_factor / lu_solve as used by lqp_py/lu_layer.py:
 * 10,31,33,52 and solve_box_qp_admm_torch.py:215,254,267.  M (B,N,N) is
 * overwritten by the packed LU (LAPACK layout), piv (B,N) int32 1-based,
 * info (B) int32: 0 or the 1-based index of the first zero pivot.          */
size_t lqp_lu_factor_workspace_bytes(int dtype, int B, int N);
int lqp_lu_factor_batched(void* stream, int dtype, int B, int N,
                          void* M_inout, int32_t* piv_out, int32_t* info_out,
                          void* workspace, size_t workspace_bytes);

/* rhs (B,N,k) overwritten by the solution.  The factor is first re-laid
 * out into solve-ordered 64x64 panels inside `workspace`.                   */
size_t lqp_lu_solve_workspace_bytes(int dtype, int B, int N);
int lqp_lu_solve_batched(void* stream, int dtype, int B, int N, int k,
                         const void* LU, const int32_t* piv, void* rhs_inout,
                         void* workspace, size_t workspace_bytes);

/* Two-step form for a factor that is reused many times (TorchLU in unroll
 * mode): pack once into `packed` (size lqp_lu_packed_bytes), solve often.   */
size_t lqp_lu_packed_bytes(int dtype, int B, int N);
int lqp_lu_pack(void* stream, int dtype, int B, int N,
                const void* LU, const int32_t* piv, void* packed);
int lqp_lu_solve_packed(void* stream, int dtype, int B, int N, int k,
                        const void* packed, void* rhs_inout);

/* ---- batched SPD inverse (f32, n <= 1024) ---------------------------------
 * Building block of linsolve 2 (the x-update x = H w + c replaces the cached LU solve of
 * solve_box_qp_admm_torch.py:267): Kinv_out (B,n,n) = K_in^-1 for symmetric positive definite K_in (B,n,n);
 * info (B) int32: 0, or 1 + index of the first non-positive pivot (K_in not positive definite).           */
size_t lqp_spd_inverse_workspace_bytes(int dtype, int B, int n);
int lqp_spd_inverse_batched(void* stream, int dtype, int B, int n, const void* K_in, void* Kinv_out,
                            int32_t* info_out, void* workspace, size_t workspace_bytes);

/* ---- equality-constrained / unconstrained QP = one KKT solve ------------
 * Replaces torch_solve_qp_eqcon (lqp_py/solve_qp_eqcon_torch.py:6-34, KKT
 * block from lqp_py/utils.py:23-32) and, with m == 0, torch_solve_qp_uncon
 * (lqp_py/solve_qp_uncon_torch.py:4-15): [[Q,A^T],[A,0]] [x;nu] = [-p;b].   */
size_t lqp_kkt_solve_workspace_bytes(int dtype, int B, int n, int m);
int lqp_kkt_solve(void* stream, int dtype, int B, int n, int m,
                  const void* Q, const void* p, const void* A, const void* b,
                  void* x, void* nus, int32_t* fail_index,
                  void* workspace, size_t workspace_bytes);

/* Symmetric rank-2 epilogue shared by the eq-con / uncon gradients
 * (solve_qp_eqcon_torch.py:57-66, solve_qp_uncon_torch.py:29-33):
 * dQ = 0.5 (dx x^T + x dx^T), dA = dnu x^T + nus dx^T (dA skipped if m==0). */
int lqp_qp_outer_grads(void* stream, int dtype, int B, int n, int m,
                       const void* dx, const void* x, const void* dnu, const void* nus,
                       void* dQ, void* dA);

#ifdef __cplusplus
}
#endif
#endif /* LQP_AMD_H */
