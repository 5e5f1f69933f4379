// Kernels of the box-QP ADMM layer (forward setup / loop / epilogue, adaptive
// rho, fixed-point backward, KKT solve).  One 1024-thread workgroup per QP.
#pragma once
#include <type_traits>
#include "lqp_common.hpp"
#include "lqp_lu.hpp"
#include "lqp_lu2.hpp"
#include "lqp_lu_wide.hpp"
#include "lqp_trsv.hpp"
#include "lqp_spd.hpp"

namespace lqp {

// ---- device-side status block (ints) ---------------------------------------
enum { ST_DONE = 0, ST_FINAL_ITER = 1, ST_GATE = 2, ST_NFACTOR = 3, ST_RHO_UPDATED = 4,
       ST_TIMEOUT = 5, ST_NCHECK = 6, ST_NOTSPD = 7,
       ST_VOTE = 8,      // 4 words: {ranks leaving the symmetric path, ranks with a singular KKT matrix, -, -} (strict global stop)
       ST_ANY_LB = 12, ST_ANY_UB = 13,      // some lower / upper bound of the batch is finite (:129-130): the per-problem
                                            // answers of k_fwd_setup (FwdParams::bflags), OR-ed by the forward's last kernel
       ST_RESUME = 14,   // the iteration at which the hot two-workgroup loop handed over to the continuation kernel (FwdParams::hot_past)
       ST_NDONE = 15,    // control['stop'] = 'each': problems that have stopped (whoever makes it B sets ST_DONE)
       ST_WORDS = 16 };
// control['stop'] = 'each' (lqp_boxqp_ctrl.reserved2 bit 3): per-problem words behind everything else in the workspace, zeroed by
// k_fwd_setup -- {stopped, iteration it stopped at (or the last one it ran), resume iteration (unused), refactorisations it made}
enum { PS_DONE = 0, PS_FINAL = 1, PS_RESUME = 2, PS_NFACTOR = 3, PS_WORDS = 4 };
// host report (lqp_boxqp_ctrl.host_report): [ST_WORDS status words as workgroup 0 of the forward's last kernel sees them |
// B info words | B flag words], written straight into pinned host memory by that kernel
enum { RP_LB = 1, RP_UB = 2, RP_TIMEOUT = 4, RP_NOTSPD = 8,
       RP_INFEAS = 1 << 16,       // control['infeasible']: the problem was flagged primal infeasible (each_stop)
       RP_UNBOUNDED = 1 << 17,    // control['unbounded']: the problem was flagged dual infeasible (each_stop)
       RP_L1_INPUT = 1 << 18,     // lqp_boxqp_forward_l1: a weight of the problem is negative or not finite, or its rho not positive (k_term_setup); its outputs are NaN
       RP_SOFT_INPUT = 1 << 19,   // lqp_boxqp_forward_soft: a weight negative or not finite, lo > hi, a NaN in lo or hi, or a rho not positive and finite (k_term_setup); its outputs are NaN
       RP_LOG_INPUT = 1 << 20,    // lqp_boxqp_forward_log: a weight negative or not finite, w_i > 0 with ub_i <= 0, or a rho not positive and finite (k_term_setup); its outputs are NaN
       RP_PWL_INPUT = 1 << 21,    // lqp_boxqp_forward_pwl: a slope not finite, slopes or kinks that decrease, a NaN kink, or a rho not positive and finite (k_term_setup); its outputs are NaN
       RP_HUBER_INPUT = 1 << 22 };  // lqp_boxqp_forward_huber: a weight negative or not finite, a delta negative or NaN, a centre not finite, or a rho not positive and finite (k_term_setup); its outputs are NaN
// per-check counters (uint32 x 4): not-optimal, arrivals, wants-rho, ratio-trigger
// (NOTOPT and ARRIVE share one aligned 64-bit word: the two-workgroup loop adds to and reads both with ONE atomic)
enum { CT_NOTOPT = 0, CT_ARRIVE = 1, CT_WANTS = 2, CT_TRIG = 3, CT_WORDS = 4 };
// verbose=True (reference :289-294: the largest primal and dual error of the batch at every check): non-negative floats order like
// their bit patterns, so one atomicMax per problem and value does it (first lap of the ring only: the trace holds `ring` checks)
template <typename T>
__device__ __forceinline__ void trace_check(unsigned int* __restrict__ vtrace, const int it, const int check_solved, const int ring,
                                            const T pri, const T dua) {
    if (!vtrace) return;
    const int c = it / check_solved;
    if (c >= ring) return;
    atomicMax(vtrace + 2 * c, __float_as_uint((float)pri));
    atomicMax(vtrace + 2 * c + 1, __float_as_uint((float)dua));
}
// per-problem scalars
enum { SC_RHO = 0, SC_PNORM = 1, SC_RATIO = 2, SC_WANTS = 3, SC_PRI = 4, SC_DUA = 5, SC_TRIG = 6, SC_WORDS = 8 };   // PRI/DUA: errors of the last check; TRIG: the ratio triggers (stop = 'each' only)

constexpr int XCHG_NPMAX = 4;                                // workgroups per QP of the shared loop, at most
constexpr int XCHG_WORDS = 2 * XCHG_NPMAX * SPD_MAXK * LQP_NB;      // exchange granules per QP of the shared loop: [parity][part][element]
// behind the granules of all QPs, per QP: [0..4) step granules of the resident sweep's workgroups | [4..8) the XCD ids its
// workgroups announce | [8..12) the same for the shared loop (XCHG_TAIL words; zeroed by the setup kernel)
constexpr int XCHG_TAIL = 12;
constexpr int DNX_WORDS = 2 * 256 * 2;   // dense LU-tier loop (lqp_dense.hpp): [parity][row <= 256][one (f32) or two (f64) words]
// the XCD this workgroup runs on (0..7)
__device__ __forceinline__ unsigned int my_xcd() { return (unsigned int)__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xFu; }

template <typename T> struct FwdParams {
    int B, n, m, N, Np, K, ldq;          // ldq: leading dim of Qs
    int Ks, sym_rl, sym_rl_hot;          // symmetric-inverse path: 64-blocks of n, LDS-resident blocks of the loop
                                         // (continuation kernel / 512-thread first launch)
    unsigned long long* dbg;             // optional cycle counters (8 per problem), debug only
    int dbg_qpass;                       // LQP_DBG_QPASS=1: the caller's debug buffer has a second half of B x 8 words for the stamps of the sweep's pass over Q
    int piv_cols;                        // 1: the resident sweep's last pivot block stops behind column n (LQP_PIV_COLS; in the alignment gap in front of the pointer: no offset moves)
    unsigned long long* dbg_setup;       // the same words for k_fwd_setup's stamps (LQP_DBG_SETUP=1: then only those)
    int spd;                             // 1: symmetric-inverse path (no KKT matrix M is assembled)
    int qs_lazy;                         // 1: the scaled matrix Qs is not stored; its readers compute (D_i Q_ij) D_j
    int eq_in_loop;                      // 1: k_admm_loop_split applies the equality correction to its register blocks (no k_spd_end)
    int hot_past;                        // 1: the persistent two-workgroup loop runs on PAST the iterations at which the reference may adapt
                                         //    rho (:237) as long as the counters of the check before say "nothing to update", leaves at one
                                         //    that does and names it in status[ST_RESUME]; the continuation launch starts there
    int hot_resume;                      // 1: this launch of the persistent two-workgroup loop starts at status[ST_RESUME] (behind a rho event
                                         //    the library handled between two launches: k_rho_update + gated refactorisation)
    int split_seg;                       // 1: k_admm_loop_split launched once per check segment for a batch LARGER than half the CUs (the
                                         //    pairs take their turns on the chip): workgroups 16 g + x and 16 g + 8 + x share problem 8 g + x
                                         //    (same XCD, neighbours in its dispatch queue), no verdict inside the kernel
    int seg_prev_slot;                   // ... counter slot of the last check before it0 (-1: none)
    int rho_late;                        // 1: rho = ||Qs||_F / sqrt(n) from the sums k_spd_begin leaves, added by k_spd_resident
    int prep_fused;                      // 3: no k_spd_prep at all -- the resident sweep reads Q itself (maxima, verdict, tiles; k_fwd_setup defers what needs D to it); 1 / 2: k_spd_prep ran BEFORE the setup kernel (2: one-workgroup tier, k_spd_inverse finishes the blocks) -- one pass over Q for the column maxima, the
                                         //    symmetry verdict and the UNSCALED blocks; the resident sweep scales them as it loads
                                         //    them and takes ||Qs||_F (-> rho) from its own tiles
    int ar_iter, ar_max, ring;           // adaptive-rho schedule and counter-ring length, for the in-kernel events
    // inputs
    const T *Q, *p, *A, *b, *lb, *ub, *rho_in, *beta_in;
    const int* bound_flags_in;           // optional {any_lb, any_ub} of a LARGER batch this call is a shard of (device), or null
    int xcd_local;                       // 1: workgroups that share a matrix and find themselves on ONE XCD exchange through its L2
    int* host_report;                    // optional pinned host memory, ST_WORDS + 2 B ints (see RP_*), or null
    int zero_words;                      // ints from `status` on (status block + counter ring) that workgroup 0 of k_fwd_setup zeroes
    // outputs
    T *x, *z, *u, *lams, *nus, *rho_out;
    // workspace
    T* Qs;            // B * n * ldq (scale) or unused
    T* M;             // B * Np * Np
    T* packed;        // B * K(K+1) * 4096
    T* vecs;          // B * vstride
    T* scal;          // B * SC_WORDS
    int* piv;         // B * Np
    int* dest;        // B * Np
    int* info;        // B
    int* bflags;      // B: RP_LB | RP_UB of problem b (k_fwd_setup)
    int* status;      // ST_WORDS
    unsigned int* counters;   // ring of CT_WORDS per check
    unsigned int* vtrace;     // nullptr, or [ring][2]: bit patterns of the largest primal / dual error over the batch per check (verbose)
    unsigned long long* xchg; // B * XCHG_WORDS granules: partial-product exchange of the two-workgroup loop (or null)
    unsigned long long* dnx;  // B * dnx_words granules: x-parts of the dense LU-tier loops, lqp_dense.hpp (or null)
    int dnx_words;            // granules per problem (DNX_WORDS, or what the W-workgroup form needs: 2 parities x n elements)
    size_t vstride;
    // controls
    int scale, rho_mode, beta_mode, check_solved, adaptive_rho;
    T eps_abs, eps_rel, rho_value, rho_min, rho_max, ar_tol, ar_inv_tol, ar_thr, beta_value;
    T alpha, alpha_c;         // over-relaxation factor (control['alpha']; 1 = the reference's plain step) and 1 - alpha, see admm_relax
    int relax;                // 1: alpha != 1
    int term;                 // the separable term of the objective, Term*::kind below: 0 none | 1 lqp_boxqp_forward_l1: sum_i w_i |x_i - c_i|
                              // | 2 lqp_boxqp_forward_soft: sum_i wl_i (lo_i - x_i)_+ + wu_i (x_i - hi_i)_+ | 3 lqp_boxqp_forward_log: -sum_i w_i log(x_i)
                              // | 4 lqp_boxqp_forward_pwl: sum_i s_i0 x_i + sum_k (s_ik - s_i,k-1) (x_i - c_ik)_+
                              // | 5 lqp_boxqp_forward_huber: sum_i w_i H_delta_i(x_i - c_i)
                              // (in the alignment gap in front of the pointer: no offset moves)
    int* pstat;              // B * PS_WORDS: control['stop'] = 'each' (every problem stops and adapts rho as a batch of one), or null
    union {
    T* snap;                 // B * snap_stride: control['infeasible'] (stop = 'each' only) -- the certificate's snapshots, or null = no detection
    T* termv;                // term != 0 (never together with the snapshots, and at their place in the workspace): the term's area,
    };                       //   B * term_stride<TERM>(n), per problem the slots its trait names; k_term_setup writes the scaled inputs
    size_t snap_stride;
    T eps_pinf;              // control['eps_prim_inf']; 0: the primal certificate is off (lqp_boxqp_forward_certify with the dual one alone)
    T eps_dinf;              // control['eps_dual_inf']; 0: no dual certificate (control['unbounded'] absent) -- the slots then end behind nu
};
// control['infeasible']: the snapshot of problem b -- (y, g, nu) of its last check, see infeas_view.  TWO slots by the parity of the check's
// number (it / check_solved): a check reads the other slot and writes its own, so the workgroups of a shared problem (k_admm_loop_split, FormEach:
// bit-identical iterates, at most one hand-off apart) write the same values and never a slot somebody still reads.
// A slot: [rho it was taken at | mark = iteration + 1 (0: none, k_snap_init) | - | - | y (n) | g (n) | nu (m)], and behind nu, with the dual
// certificate alone (control['unbounded'], `dual`): [x (n) | qx (n)], qx = Qs x -- see dinf_elem
enum { SN_RHO = 0, SN_MARK = 1, SN_HEAD = 4 };
__host__ __device__ inline size_t snap_slot_len(int n, int m, bool dual = false) { return (size_t)round_up(SN_HEAD + 2 * n + m + (dual ? 2 * n : 0), 4); }
__host__ __device__ inline size_t snap_stride(int n, int m, bool dual = false) { return 2 * snap_slot_len(n, m, dual); }

// vector block of problem b: [ps | lbs | ubs | D | z | u | x | As (m*n) | bs | E | nu | cv | Tm (m*n) | s0]
// (cv, Tm, s0: constant term c, T = G S^-1 and S^-1 b of the symmetric-inverse path, lqp_spd.hpp)
template <typename T> struct VecView {
    T *ps, *lbs, *ubs, *D, *z, *u, *x, *As, *bs, *E, *nu, *cv, *Tm, *s0;
    __device__ VecView(T* base, int n, int m) {
        ps = base; lbs = ps + n; ubs = lbs + n; D = ubs + n; z = D + n; u = z + n; x = u + n;
        As = x + n; bs = As + (size_t)m * n; E = bs + m; nu = E + m;
        cv = nu + m; Tm = cv + n; s0 = Tm + (size_t)m * n;
    }
};
__host__ __device__ inline size_t vec_stride(int n, int m) { return (size_t)round_up(8 * n + 2 * m * n + 4 * m, 8); }

// ---------------------------------------------------------------------------
// setup: norms, auto-scaling, rho, KKT assembly, state init
// (lqp_py/solve_box_qp_admm_torch.py:124-131, 160-212, 221-223)
// LDS: red[NW * n] | d[n] | sel[8] | scratch[NW]
// ---------------------------------------------------------------------------
// (n <= 1024: one slab of column maxima per wave; above, the waves merge their maxima into 4 slabs in 4 rounds -- 16
//  slabs of 2048 doubles would not fit)
__host__ __device__ inline int setup_slabs(int n) { return n > 1024 ? 4 : LQP_NW; }
template <typename T> __host__ __device__ inline int setup_lds_bytes(int n) {
    return (round_up(setup_slabs(n) * n, 8) + round_up(n, 8) + 8 + LQP_NW + 8) * (int)sizeof(T);
}

// M = [[Qs + rho I, As^T], [As, 0]]  (solve_box_qp_admm_torch.py:206-212, 252).
// copy_q == false: the top-left block already holds Qs (written by the scaling pass), only
// rho is added on the diagonal.
template <typename T>
__device__ __forceinline__ void assemble_kkt_rows(const FwdParams<T>& P, const int b, const T* __restrict__ Qs, const int ldq,
                                                  const VecView<T>& V, const T rho, const bool copy_q,
                                                  const T* __restrict__ dsc = nullptr) {
    // dsc != nullptr: `Qs` is the UNSCALED matrix and dsc the scaling vector (FwdParams::qs_lazy on the LU path: the scaled matrix
    // is not kept for the refactorisations, they form (D_i Q_ij) D_j again -- the expression of the setup pass, the same bits)
    const int n = P.n, m = P.m, Np = P.Np;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T* M = P.M + (size_t)b * Np * Np;
    typedef V4<T> vec;
    const bool vec_ok = (ldq % 4 == 0) && ((((uintptr_t)Qs) % sizeof(vec)) == 0) && (n % 4 == 0 || dsc == nullptr);
    if (copy_q) {
        for (int i = w; i < n; i += LQP_NW) {
            const T* q = Qs + (size_t)i * ldq;
            T* mr = M + (size_t)i * Np;
            const T di = dsc ? dsc[i] : T(1);
            if (vec_ok) {
                for (int j = lane * 4; j < n; j += 256) {
                    if (j + 3 < n) {
                        vec v = *(const vec*)(q + j);
                        if (dsc) {
                            const vec dj = *(const vec*)(dsc + j);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v.v[e] = (di * v.v[e]) * dj.v[e];
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (j + e == i) v.v[e] += rho;
                        *(vec*)(mr + j) = v;
                    } else {
                        for (int e = 0; e < 4 && j + e < n; ++e)
                            mr[j + e] = (dsc ? (di * q[j + e]) * dsc[j + e] : q[j + e]) + (i == j + e ? rho : T(0));
                    }
                }
            } else {
                for (int j = lane; j < n; j += 64) mr[j] = (dsc ? (di * q[j]) * dsc[j] : q[j]) + (i == j ? rho : T(0));
            }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += LQP_NT) M[(size_t)i * Np + i] += rho;
    }
    for (int i = w; i < n; i += LQP_NW) {
        T* mr = M + (size_t)i * Np;
        for (int r = lane; r < m; r += 64) mr[n + r] = V.As[(size_t)r * n + i];
    }
    for (int r = w; r < m; r += LQP_NW) {
        T* mr = M + (size_t)(n + r) * Np;
        for (int j = lane; j < n; j += 64) mr[j] = V.As[(size_t)r * n + j];
        for (int c = lane; c < m; c += 64) mr[n + c] = T(0);
    }
}

// ---- the two passes of the scaling over Q (16-B row pieces).  NQ: column quads of 256 per lane, RIF: rows in
//      flight per wave.  Loads are UNCONDITIONAL (lanes past the row end re-read column 0 and their values are masked
//      out): a per-lane `if (j < n)` around a load becomes a branch with s_waitcnt vmcnt(0) right behind it, i.e. one
//      1-KB load in flight per wave.  All RIF rows' loads are issued before any is used. ----
template <typename T, int NQ, int RIF>
__device__ __forceinline__ void setup_colmax(const T* __restrict__ Q, const int n, T* __restrict__ red) {
    const int row0 = 0, row1 = n;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    T cm[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) cm[q][e] = T(0);
    const int nq = (n + 255) / 256;               // column quads of 256 that exist (uniform)
    int jq[NQ]; bool okq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { const int j = (lane + 64 * q) * 4; okq[q] = j < n; jq[q] = okq[q] ? j : 0; }
    for (int i0 = row0 + w; i0 < row1; i0 += RIF * LQP_NW) {
        V4<T> v[RIF][NQ];
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr) {
            const int i = i0 + rr * LQP_NW;
            const T* qr = Q + (size_t)(i < row1 ? i : i0) * n;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < nq) v[rr][q] = *(const V4<T>*)(qr + jq[q]);
        }
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q < nq) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) cm[q][e] = tmax(cm[q][e], okq[q] ? tabs(v[rr][q].v[e]) : T(0));
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int j = (lane + 64 * q) * 4;
        if (j < n) {
#pragma unroll
            for (int e = 0; e < 4; ++e) red[(size_t)w * n + j + e] = cm[q][e];
        }
    }
}
// Qs = (D_i Q_ij) D_j (and the top-left KKT block when with_m); returns this thread's share of ||Qs||_F^2
template <typename T, int NQ, int RIF>
__device__ __forceinline__ T setup_scale(const T* __restrict__ Q, const int n, const T* __restrict__ d, T* __restrict__ Qw,
                                         const int ldq, T* __restrict__ Mw, const int Np, const bool with_m) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nq = (n + 255) / 256;
    int jq[NQ]; bool okq[NQ]; V4<T> dj[NQ];
    T fro2 = T(0);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int j = (lane + 64 * q) * 4;
        okq[q] = j < n; jq[q] = okq[q] ? j : 0;
        dj[q] = *(const V4<T>*)(d + jq[q]);
    }
    for (int i0 = w; i0 < n; i0 += RIF * LQP_NW) {
        V4<T> v[RIF][NQ];
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr) {
            const int i = i0 + rr * LQP_NW;
            const T* qr = Q + (size_t)(i < n ? i : i0) * n;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < nq) v[rr][q] = *(const V4<T>*)(qr + jq[q]);
        }
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr) {
            const int i = i0 + rr * LQP_NW;
            if (i < n) {
                T* qo = Qw + (size_t)i * ldq;
                T* mo = Mw + (size_t)i * Np;
                const T di = d[i];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    if (q < nq && okq[q]) {
                        V4<T> o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { o.v[e] = (di * v[rr][q].v[e]) * dj[q].v[e]; fro2 += o.v[e] * o.v[e]; }
                        if (Qw) *(V4<T>*)(qo + jq[q]) = o;
                        if (with_m) *(V4<T>*)(mo + jq[q]) = o;
                    }
                }
            }
        }
    }
    return fro2;
}

// The same two passes for rows that are not 16-B pieces (n % 4 != 0, e.g. the hard distribution's n = 250): NC column groups
// of 64 per lane, one element each, RIF rows in flight; unconditional loads at clamped columns as above.  (The plain loop
// with a per-lane `if (j < n)` had one 512-B load in flight per wave: 64 MB in 33 us at n = 250 in float64.)
template <typename T, int NC, int RIF>
__device__ __forceinline__ void setup_colmax_s(const T* __restrict__ Q, const int n, T* __restrict__ red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = (n + 63) / 64;
    T cm[NC];
    int jq[NC]; bool okq[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) { const int j = lane + 64 * q; okq[q] = j < n; jq[q] = okq[q] ? j : 0; cm[q] = T(0); }
    for (int i0 = w; i0 < n; i0 += RIF * LQP_NW) {
        T v[RIF][NC];
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr) {
            const int i = i0 + rr * LQP_NW;
            const T* qr = Q + (size_t)(i < n ? i : i0) * n;
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (q < nq) v[rr][q] = qr[jq[q]];
        }
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr)
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (q < nq) cm[q] = tmax(cm[q], okq[q] ? tabs(v[rr][q]) : T(0));
    }
#pragma unroll
    for (int q = 0; q < NC; ++q)
        if (okq[q]) red[(size_t)w * n + lane + 64 * q] = cm[q];
}
template <typename T, int NC, int RIF>
__device__ __forceinline__ T setup_scale_s(const T* __restrict__ Q, const int n, const T* __restrict__ d, T* __restrict__ Qw,
                                           const int ldq, T* __restrict__ Mw, const int Np, const bool with_m) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = (n + 63) / 64;
    int jq[NC]; bool okq[NC]; T dj[NC];
    T fro2 = T(0);
#pragma unroll
    for (int q = 0; q < NC; ++q) { const int j = lane + 64 * q; okq[q] = j < n; jq[q] = okq[q] ? j : 0; dj[q] = d[jq[q]]; }
    for (int i0 = w; i0 < n; i0 += RIF * LQP_NW) {
        T v[RIF][NC];
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr) {
            const int i = i0 + rr * LQP_NW;
            const T* qr = Q + (size_t)(i < n ? i : i0) * n;
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (q < nq) v[rr][q] = qr[jq[q]];
        }
#pragma unroll
        for (int rr = 0; rr < RIF; ++rr) {
            const int i = i0 + rr * LQP_NW;
            if (i < n) {
                T* qo = Qw + (size_t)i * ldq;
                T* mo = Mw + (size_t)i * Np;
                const T di = d[i];
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    if (q < nq && okq[q]) {
                        const T o = (di * v[rr][q]) * dj[q];
                        fro2 += o * o;
                        if (Qw) qo[jq[q]] = o;
                        if (with_m) mo[jq[q]] = o;
                    }
                }
            }
        }
    }
    return fro2;
}

// scratch of k_spd_prep for problem b (the Qs area: unused while the scaled matrix is not stored):
// [SPD_NP][64 Ks] column maxima | [SPD_NP] ints: symmetry verdicts
template <typename T>
__device__ __forceinline__ T* prep_scratch(const FwdParams<T>& P, const int b) { return P.Qs + (size_t)b * P.n * P.ldq; }

// The auto-scaling vector (reference :163-175) from the column maxima of |Q|: red[ww * n + j], ww < nred (LDS; reused as the
// sort buffer) -> d[0..n) (LDS).  Zero guard, D = sqrt(1 / max), beta from the 10 % / 90 % quantiles of D, the blend with the
// mean.  A workgroup of NT threads (k_fwd_setup: 1024; the resident sweep, which takes the maxima from its own pass over Q:
// 512 -- for n <= 512 every thread holds the same element in both and the sums are taken in the same order: the same bits).
// sel: 8 elements, scratch: >= NT / 64 (LDS).
template <typename T, int NT>
__device__ __forceinline__ void wg_scaling_vector(const FwdParams<T>& P, const int b, T* __restrict__ red, const int nred,
                                                  T* __restrict__ d, T* __restrict__ sel, T* __restrict__ scratch) {
    const int tid = threadIdx.x, n = P.n;
    T part = T(0);
    for (int j = tid; j < n; j += NT) {
        T v = red[j];
        for (int ww = 1; ww < nred; ++ww) v = tmax(v, red[(size_t)ww * n + j]);
        d[j] = v;
        part += v;
    }
    // ---- zero guard (:164-168) ----
    const T mean_norm = wg_sum_nw<NT / 64>(part, scratch) / T(n);
    const T floor_v = tmax(mean_norm, T(1e-6));
    part = T(0);
    for (int j = tid; j < n; j += NT) {
        T v = d[j];
        if (v <= T(0)) v = tmax(v, floor_v);
        v = tsqrt(T(1) / v);          // D = sqrt(1 / Q_norm) (:170)
        d[j] = v;
        part += v;
    }
    const T dmean = wg_sum_nw<NT / 64>(part, scratch) / T(n);     // also makes d[] visible
    // ---- beta = 1 - q10(D) / q90(D), linear-interpolated quantiles (:171-174) ----
    T beta = P.beta_mode == 2 ? P.beta_in[b] : P.beta_value;
    if (P.beta_mode == 0) {
        const T pos0 = T(0.10) * T(n - 1), pos1 = T(0.90) * T(n - 1);
        const int lo0 = (int)tfloor(pos0), hi0 = (int)tceil(pos0);
        const int lo1 = (int)tfloor(pos1), hi1 = (int)tceil(pos1);
        // the four order statistics behind the two quantiles: bitonic sort of D, padded with +inf to a power of two.
        // One element per thread while that fits: partners closer than 64 are reached by a wave shuffle, only the
        // far ones (6 of the 45 rounds at n = 500) go through LDS and a barrier.  (Counting every element's rank
        // costs n^2 comparisons: 10 us at n = 500 even over all 1024 threads; every round through LDS: 12 us.)
        T* sb = red;                                      // the column maxima are no longer needed
        int N2 = 1;
        while (N2 < n) N2 <<= 1;
        __syncthreads();
        if (N2 <= NT) {
            T v = tid < n ? d[tid] : T(INFINITY);
            for (int k = 2; k <= N2; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    T other;
                    if (j >= 64) {
                        if (tid < N2) sb[tid] = v;
                        __syncthreads();
                        other = tid < N2 ? sb[tid ^ j] : v;
                        __syncthreads();
                    } else {
                        other = __shfl_xor(v, j);
                    }
                    const bool keep_min = ((tid & j) == 0) == ((tid & k) == 0);
                    v = keep_min ? tmin(v, other) : tmax(v, other);
                }
            }
            if (tid < N2) sb[tid] = v;
            __syncthreads();
        } else {
            for (int i = tid; i < N2; i += NT) sb[i] = i < n ? d[i] : T(INFINITY);
            __syncthreads();
            for (int k = 2; k <= N2; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < (N2 >> 1); t += NT) {
                        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                        const T x0 = sb[i], x1 = sb[l];
                        if ((x0 > x1) == ((i & k) == 0)) { sb[i] = x1; sb[l] = x0; }
                    }
                    __syncthreads();
                }
            }
        }
        if (tid == 0) { sel[0] = sb[lo0]; sel[1] = sb[hi0]; sel[2] = sb[lo1]; sel[3] = sb[hi1]; }
        __syncthreads();
        const T w0 = pos0 - tfloor(pos0), w1 = pos1 - tfloor(pos1);
        // torch lerp: w < 0.5 ? a + w (b - a) : b - (b - a)(1 - w)
        const T q10 = (w0 < T(0.5)) ? sel[0] + w0 * (sel[1] - sel[0]) : sel[1] - (sel[1] - sel[0]) * (T(1) - w0);
        const T q90 = (w1 < T(0.5)) ? sel[2] + w1 * (sel[3] - sel[2]) : sel[3] - (sel[3] - sel[2]) * (T(1) - w1);
        beta = T(1) - q10 / q90;
    }
    __syncthreads();
    for (int j = tid; j < n; j += NT) {
        const T v = (T(1) - beta) * d[j] + beta * dmean;     // (:175)
        d[j] = v;
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_fwd_setup(const FwdParams<T> P) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, n = P.n, m = P.m, Np = P.Np;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    T* red = (T*)smem;
    T* d = red + (size_t)round_up(setup_slabs(n) * n, 8);
    T* sel = d + round_up(n, 8);
    T* scratch = sel + 8;
    const T* Q = P.Q + (size_t)b * n * n;
    const T* p = P.p + (size_t)b * n;
    VecView<T> V(P.vecs + (size_t)b * P.vstride, n, m);
    T* scal = P.scal + (size_t)b * SC_WORDS;
    if (tid == 0) P.info[b] = 0;
    // status block + counter ring start from zero.  Nobody else in this launch touches them (the bound flags are per
    // problem, see below), every later launch is ordered behind this one: no separate fill launch (3.6 us + a boundary).
    if (b == 0)
        for (int i = tid; i < P.zero_words; i += LQP_NT) P.status[i] = 0;
    if (P.pstat && tid < PS_WORDS) P.pstat[(size_t)b * PS_WORDS + tid] = 0;      // (stop = 'each': every workgroup its own words)
    unsigned long long tst = clock64();
#define SETUP_STAMP(i) do { if (P.dbg_setup && tid == 0) { const unsigned long long t_ = clock64(); P.dbg_setup[(size_t)b * 8 + (i)] = t_ - tst; tst = t_; } } while (0)
    if (P.dnx) {                           // granules of the dense LU-tier loop (lqp_dense.hpp): tags start from zero
        unsigned long long* dq = P.dnx + (size_t)b * P.dnx_words;
        for (int i = tid; i < P.dnx_words; i += LQP_NT) dq[i] = 0ull;
    }
    if (P.xchg) {                          // exchange granules of the two-workgroup loop: tags start from zero
        unsigned long long* xq = P.xchg + (size_t)b * XCHG_WORDS;
        for (int i = tid; i < XCHG_WORDS; i += LQP_NT) xq[i] = 0ull;
        if (tid < XCHG_TAIL) P.xchg[(size_t)P.B * XCHG_WORDS + XCHG_TAIL * b + tid] = 0ull;      // step granules of the resident sweep, XCD announcements
    }

    // the small vectors are requested now and used after the pass over Q (n <= 1024: one element per thread; a load
    // issued where it is needed costs a full memory latency each time, ~2 us, with nothing to hide it behind)
    const T* lb = P.lb + (size_t)b * n;
    const T* ub = P.ub + (size_t)b * n;
    const T p0 = tid < n ? p[tid] : T(0), lb0 = tid < n ? lb[tid] : T(0), ub0 = tid < n ? ub[tid] : T(0);
    const T a0 = (m > 0 && tid < n) ? P.A[(size_t)b * m * n + tid] : T(0);          // first equality row
    SETUP_STAMP(0);
    const T* Qs = Q;
    int ldq = n;
    T fro2 = T(0);
    bool q_in_m = false;          // top-left KKT block already written by the scaling pass
    // prep_fused == 3: the resident sweep makes the pass over Q itself (column maxima, symmetry verdict, tiles straight into
    // its registers) and with it everything that needs D: the vector, ps, As / E / bs, lbs / ubs (wg_deferred_*).  What is
    // left here: the zeroes, ||p||_inf, a given rho, the bound flags.
    const bool defer = P.prep_fused == 3;
    if (defer) {
    } else if (P.scale) {
        // ---- column max of |Q| (:163): wave w sweeps rows w, w+16, ...; 16 B per lane per load ----
        const bool qvec = (n % 4 == 0) && n <= 1024 && ((((uintptr_t)Q) % sizeof(V4<T>)) == 0);
        int nred = LQP_NW;
        if (P.prep_fused) {
            // k_spd_prep has been over Q: the maxima of its SPD_NP workgroups' shares, and their symmetry verdicts
            const T* cmp = prep_scratch(P, b);
            for (int j = tid; j < n; j += LQP_NT) red[j] = tmax(cmp[j], cmp[P.Ks * LQP_NB + j]);
            if (tid == 0 && (((const int*)(cmp + 2 * P.Ks * LQP_NB))[0] | ((const int*)(cmp + 2 * P.Ks * LQP_NB))[1]) != 0)
                P.info[b] = P.Ks * 64 + 2;           // not symmetric: the LU path takes it (status word: set by the loop kernel)
            nred = 1;
        } else if (qvec) {
            // (several workgroups per QP for this pass: no faster -- 128 MB in 38 us either way, the HBM rate)
            // (up to 256 columns: one 16-B piece per lane and row -- more rows in flight instead; float64 at n = 250 had ONE 2-KB row in
            //  flight per wave: 64 MB in 33 us)
            if (n <= 256) setup_colmax<T, 1, sizeof(T) == 8 ? 4 : 8>(Q, n, red);
            else setup_colmax<T, 4, sizeof(T) == 8 ? 1 : 4>(Q, n, red);        // (8 rows in flight with 2 column quads: no faster; float64: 4 rows in flight = 128 VGPRs of loads, 315 spilled registers)
        } else if (n <= 256) {
            setup_colmax_s<T, 4, 4>(Q, n, red);
        } else if (n <= 512) {
            setup_colmax_s<T, 8, 2>(Q, n, red);
        } else {
            // (also the HBM-resident tier, 1024 < n <= 2048: two passes of 1024 columns, the 16 waves merging their maxima
            //  into setup_slabs(n) = 4 slabs in 4 rounds; up to 1024 columns: one pass, one slab per wave, no round trip)
            nred = setup_slabs(n);
            for (int c0 = 0; c0 < n; c0 += 1024) {
                T cm[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) cm[q] = T(0);
                // (unconditional loads, eight in flight per wave -- lanes past the row end re-read its first column and are masked: a guarded load
                //  is a branch with a full wait behind it, one 256-B load in flight per wave: 9 MB in 0.6 ms at n = 1500)
                for (int i = w; i < n; i += LQP_NW) {
                    const T* qr = Q + (size_t)i * n + c0;
                    if constexpr (sizeof(T) == 4) {
#pragma unroll
                        for (int h = 0; h < 16; h += 8) {
                            T v[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) { const int j = lane + 64 * (h + q); v[q] = qr[(c0 + j < n) ? j : 0]; }
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int j = lane + 64 * (h + q);
                                cm[h + q] = tmax(cm[h + q], (c0 + j < n) ? tabs(v[q]) : T(0));
                            }
                        }
                    } else {                                      // (float64: the unconditional form spills registers in this kernel)
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int j = lane + 64 * q;
                            if (c0 + j < n) cm[q] = tmax(cm[q], tabs(qr[j]));
                        }
                    }
                }
                for (int round = 0; round < LQP_NW / nred; ++round) {
                    if (w / nred == round) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int j = c0 + lane + 64 * q;
                            if (j < n) {
                                T* slot = red + (size_t)(w % nred) * n + j;
                                *slot = round == 0 ? cm[q] : tmax(*slot, cm[q]);
                            }
                        }
                    }
                    if (nred < LQP_NW) __syncthreads();
                }
            }
        }
        __syncthreads();
        SETUP_STAMP(1);
        wg_scaling_vector<T, LQP_NT>(P, b, red, nred, d, sel, scratch);
        SETUP_STAMP(2);
        for (int j = tid; j < n; j += LQP_NT) V.D[j] = d[j];
        SETUP_STAMP(3);
        // ---- Qs = (D_i Q_ij) D_j, its Frobenius norm (:176, :201), and the top-left KKT block ----
        ldq = P.ldq;
        // (symmetric path: the scaled matrix is not stored, its readers scale Q as they load it)
        T* Qw = P.qs_lazy ? nullptr : P.Qs + (size_t)b * n * ldq;
        T* Mw = P.M + (size_t)b * Np * Np;
        if (P.qs_lazy && P.spd && (P.rho_late || (P.prep_fused && P.rho_mode != 0) || P.prep_fused == 2)) {
            // nothing to store here and the norm (when rho is derived from it) is taken by k_spd_begin / the resident
            // sweep: no second pass over Q
        } else if (qvec) {
            // (every thread meets its elements in the same order whatever the shape of the pass: the norm keeps its bits)
            if (n <= 256) fro2 += setup_scale<T, 1, sizeof(T) == 8 ? 4 : 8>(Q, n, d, Qw, ldq, Mw, Np, !P.spd);
            else fro2 += setup_scale<T, 4, sizeof(T) == 8 ? 1 : 4>(Q, n, d, Qw, ldq, Mw, Np, !P.spd);
        } else if (n <= 256) {
            fro2 += setup_scale_s<T, 4, 4>(Q, n, d, Qw, ldq, Mw, Np, !P.spd);
        } else if (n <= 512) {
            fro2 += setup_scale_s<T, 8, 2>(Q, n, d, Qw, ldq, Mw, Np, !P.spd);
        } else {
            for (int i = w; i < n; i += LQP_NW) {
                const T* qr = Q + (size_t)i * n;
                T* qo = Qw + (size_t)i * ldq;
                T* mo = Mw + (size_t)i * Np;
                const T di = d[i];
                // (eight / four loads in flight; every lane meets its elements in the order it always did: the norm keeps its bits)
                constexpr int SQ = sizeof(T) == 8 ? 4 : 8;
                for (int j0 = lane; j0 < n; j0 += 64 * SQ) {
                    T qv[SQ];
#pragma unroll
                    for (int q = 0; q < SQ; ++q) { const int j = j0 + 64 * q; qv[q] = qr[j < n ? j : lane]; }
#pragma unroll
                    for (int q = 0; q < SQ; ++q) {
                        const int j = j0 + 64 * q;
                        if (j < n) {
                            const T v = (di * qv[q]) * d[j];
                            if (Qw) qo[j] = v;
                            if (!P.spd) mo[j] = v;
                            fro2 += v * v;
                        }
                    }
                }
            }
        }
        q_in_m = true;
        Qs = Qw;
        for (int i = tid; i < n; i += LQP_NT) V.ps[i] = d[i] * (i == tid ? p0 : p[i]);       // (:177)
    } else {
        for (int i = tid; i < n; i += LQP_NT) { V.D[i] = T(1); V.ps[i] = i == tid ? p0 : p[i]; }
        if (P.rho_mode == 0 && !(P.rho_late && P.spd)) {
            for (int i = w; i < n; i += LQP_NW) {
                const T* qr = Q + (size_t)i * n;
                for (int j = lane; j < n; j += 64) { const T v = qr[j]; fro2 += v * v; }
            }
        }
    }
    SETUP_STAMP(4);
    // ---- ||p||_inf on the unscaled p (:127) ----
    {
        T pm = tabs(p0);
        for (int i = tid + LQP_NT; i < n; i += LQP_NT) pm = tmax(pm, tabs(p[i]));
        pm = wg_max(pm, scratch);
        if (tid == 0) scal[SC_PNORM] = pm;
    }
    // ---- rho (:140, :157-158, :200-203) ----
    T rho;
    if (P.rho_mode == 0) {
        const T fro = tsqrt(wg_sum(fro2, scratch));
        rho = fro / T(sqrt((double)n));
        rho = tmin(tmax(rho, P.rho_min), P.rho_max);
    } else if (P.rho_mode == 1) {
        rho = P.rho_value;
    } else {
        rho = P.rho_in[b];
    }
    if (tid == 0) { scal[SC_RHO] = rho; scal[SC_RATIO] = T(1); scal[SC_WANTS] = T(0); }

    // ---- equality block: A D, row normalisation E (:179-190) ----
    if (m > 0 && !defer) {
        const T* A = P.A + (size_t)b * m * n;
        const T* bb = P.b + (size_t)b * m;
        if (P.scale && m >= 4 && m <= 64 && setup_slabs(n) * n >= 64) {
            // a row per wave (rows w, w + 16, ...), its norm a wave maximum, ONE barrier for the mean of the norms (a row per
            // round of the whole workgroup was three barriers a row: 42 us at m = 16; kept below four rows, where a row on one wave is slower).  The maxima are exact and the mean adds
            // them in row order as it always did: same bits.
            T* rn = red;                                   // (the column maxima are done with)
            for (int r = w; r < m; r += LQP_NW) {
                T am = T(0);
                for (int j = lane; j < n; j += 64) {
                    const T v = ((r == 0 && j == tid) ? a0 : A[(size_t)r * n + j]) * d[j];
                    am = tmax(am, tabs(v));
                }
                am = wave_max(am);
                if (lane == 0) rn[r] = am;
            }
            __syncthreads();
            T esum = T(0);
            for (int r = 0; r < m; ++r) esum += rn[r];
            const T floor_a = tmax(esum / T(m), T(1e-6));
            for (int r = w; r < m; r += LQP_NW) {
                T an = rn[r];
                if (an <= T(0)) an = tmax(an, floor_a);
                const T e = T(1) / an;
                for (int j = lane; j < n; j += 64) {
                    const T v = ((r == 0 && j == tid) ? a0 : A[(size_t)r * n + j]) * d[j];
                    V.As[(size_t)r * n + j] = e * v;
                }
                if (lane == 0) { V.E[r] = e; V.bs[r] = e * bb[r]; }
            }
            __syncthreads();
        } else if (P.scale) {
            T esum = T(0);
            for (int r = 0; r < m; ++r) {
                T am = T(0);
                for (int j = tid; j < n; j += LQP_NT) {
                    const T v = ((r == 0 && j == tid) ? a0 : A[(size_t)r * n + j]) * d[j];
                    V.As[(size_t)r * n + j] = v;
                    am = tmax(am, tabs(v));
                }
                am = wg_max(am, scratch);
                if (tid == 0) V.E[r] = am;      // row norm for now
                esum += am;
            }
            __syncthreads();
            const T floor_a = tmax(esum / T(m), T(1e-6));
            for (int r = 0; r < m; ++r) {
                T an = V.E[r];
                if (an <= T(0)) an = tmax(an, floor_a);
                const T e = T(1) / an;
                for (int j = tid; j < n; j += LQP_NT) V.As[(size_t)r * n + j] = e * V.As[(size_t)r * n + j];
                __syncthreads();
                if (tid == 0) { V.E[r] = e; V.bs[r] = e * bb[r]; }
            }
        } else {
            for (int t = tid; t < m * n; t += LQP_NT) V.As[t] = A[t];
            for (int r = tid; r < m; r += LQP_NT) { V.E[r] = T(1); V.bs[r] = bb[r]; }
        }
    }
    SETUP_STAMP(5);
    // ---- bounds (:192-194) and state ----
    // any finite bound in the batch?  (:129-130: a HOST decision in the reference -- it selects the rho = 0 shortcut and
    // the clamps.  Here the clamps always run (an infinite bound is an exact no-op) and the answer goes back with the
    // status: one word per problem here, OR-ed over the batch by the forward's last kernel (fwd_finish); the host compares
    // it with what it assumed when it chose the schedule.)
    {
        bool flb = false, fub = false;
        for (int i = tid; i < n; i += LQP_NT) {
            flb |= (i == tid ? lb0 : lb[i]) > -T(INFINITY);
            fub |= (i == tid ? ub0 : ub[i]) < T(INFINITY);
        }
        const int wg_lb = __syncthreads_or(flb ? 1 : 0), wg_ub = __syncthreads_or(fub ? 1 : 0);
        if (tid == 0) P.bflags[b] = (wg_lb ? RP_LB : 0) | (wg_ub ? RP_UB : 0);
    }
    for (int i = tid; i < n; i += LQP_NT) {
        if (!defer) {
            const T di = P.scale ? V.D[i] : T(1);                // (:192-194; +-inf / D stays +-inf)
            V.lbs[i] = (i == tid ? lb0 : lb[i]) / di;
            V.ubs[i] = (i == tid ? ub0 : ub[i]) / di;
        }
        V.z[i] = T(0); V.u[i] = T(0); V.x[i] = T(0);
    }
    for (int r = tid; r < m; r += LQP_NT) V.nu[r] = T(0);
    __syncthreads();
    SETUP_STAMP(6);
    if (!P.spd) assemble_kkt_rows(P, b, Qs, ldq, V, rho, !q_in_m);
}

// ---------------------------------------------------------------------------
// LU and pack kernels (gated: *gate == 0 -> nothing to do)
// ---------------------------------------------------------------------------
template <typename T, int PB, bool MFMA, int NT>
__global__ __launch_bounds__(NT) void k_lu_factor(T* __restrict__ Mall, const int N, const int ld,
                                                      const size_t mstride, int* __restrict__ piv,
                                                      const int pstride, int* __restrict__ info,
                                                      const int* __restrict__ gate,
                                                      unsigned long long* __restrict__ dbg,
                                                      const int* __restrict__ Nvec) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) info[b] = 0;
    __syncthreads();
    const int Nb = Nvec ? Nvec[b] : N;            // per-problem size (reduced backward systems)
    wg_lu_factor<T, PB, MFMA, NT>(Mall + (size_t)b * mstride, Nb, ld, piv + (size_t)b * pstride, info + b, smem,
                              dbg ? dbg + (size_t)b * 4 : nullptr);
}

// two workgroups per matrix (lqp_lu2.hpp; N <= 512, 2 B workgroups resident): workgroups b and b + B share matrix b
template <typename T, int PB>
__global__ __launch_bounds__(LU2_NT) void k_lu_factor2(T* __restrict__ Mall, const int N, const int ld, const size_t mstride,
                                                       int* __restrict__ piv, const int pstride, int* __restrict__ info,
                                                       const int* __restrict__ gate, const int* __restrict__ Nvec,
                                                       unsigned long long* __restrict__ scr, const size_t scr_stride,
                                                       const unsigned int epoch, unsigned long long* __restrict__ dbg,
                                                       const int B, const int xlocal_ok) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    int b, me;
    if (!shared_map((int)blockIdx.x, B, 2, b, me)) return;
    const int Nb = Nvec ? Nvec[b] : N;
    if (threadIdx.x == 0 && me == 0) info[b] = 0;
    __syncthreads();
    wg_lu_factor2<T, PB>(Mall + (size_t)b * mstride, Nb, ld, piv + (size_t)b * pstride, info + b, smem, me,
                         scr + (size_t)b * scr_stride, epoch, xlocal_ok != 0, (dbg && me == 0) ? dbg + (size_t)b * 16 : nullptr);
}

// 1024 < N <= 2048: two panel rows per thread; to 4096 in float32: four (wg_lu_factor with R > 1; no debug counters)
template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_lu_factor_big(T* __restrict__ Mall, const int N, const int ld,
                                                          const size_t mstride, int* __restrict__ piv,
                                                          const int pstride, int* __restrict__ info,
                                                          const int* __restrict__ gate, const int* __restrict__ Nvec) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) info[b] = 0;
    __syncthreads();
    // (N is the launch's size, the LDS layout follows it: a smaller Nvec[b] runs on the same form)
    if constexpr (sizeof(T) == 4) {
        if (N > 2048) {           // 2048 < N <= 4096: four rows per thread, panels of 4 columns (2 * 4 * N floats of LDS)
            wg_lu_factor<T, 4, true, LQP_NT, 4>(Mall + (size_t)b * mstride, Nvec ? Nvec[b] : N, ld, piv + (size_t)b * pstride, info + b, smem, nullptr);
            return;
        }
    }
    wg_lu_factor<T, lu_big_panel<T>(), true, LQP_NT, 2>(Mall + (size_t)b * mstride, Nvec ? Nvec[b] : N, ld,
                                                        piv + (size_t)b * pstride, info + b, smem, nullptr);
}

template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_pack(const T* __restrict__ LUall, const int N, const int ld,
                                                 const size_t mstride, const int* __restrict__ piv,
                                                 const int pstride, T* __restrict__ packed,
                                                 const size_t pkstride, int* __restrict__ dest,
                                                 const int dstride, const int vec_ok,
                                                 const int* __restrict__ gate, const int* __restrict__ Nvec) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    const int b = blockIdx.x;
    // gridDim.y == 2: two workgroups per factor (L half / U half) -- at B <= 128 half the CUs are idle
    const int part = gridDim.y == 2 ? 1 + (int)blockIdx.y : 0;
    wg_pack_factor<T>(LUall + (size_t)b * mstride, Nvec ? Nvec[b] : N, ld, piv + (size_t)b * pstride,
                      packed + (size_t)b * pkstride, dest + (size_t)b * dstride, smem, vec_ok != 0, part);
}

// ---------------------------------------------------------------------------
// ADMM loop: iterations [it0, it1) for every problem (:235-313)
// LDS: v[Np] | tmp[64] | z[n] | u[n] | ps[n] | lb[n] | ub[n] | D[n] | bs[m] | red[NW*8] | dest[Np] (int)
// ---------------------------------------------------------------------------
template <typename T> __host__ __device__ inline int loop_lds_bytes(int n, int m, int Np, bool resident) {
    return (resident ? LQP_RLDS * LQP_BLK * (int)sizeof(T) : 0) +
           (Np + 64 + 6 * n + m + LQP_NW * 8 + 8) * (int)sizeof(T) + Np * 4;
}
// residency applies when the stream is long enough and the ring can stay cyclic over the streamed tail
template <int NT> __host__ __device__ inline bool loop_resident_ok(int K, size_t elem) {
    const int S = K * (K + 1), R0 = resident_total<NT>();
    return elem == 4 && S >= R0 + LQP_PF && ((S - R0) % LQP_PF) == 0;
}

template <typename T, int NV, int NWV = LQP_NW>
__device__ __forceinline__ void wg_max_n(T (&v)[NV], T* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = wave_max(v[q]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) red[w * 8 + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        T r = red[q];
#pragma unroll
        for (int ww = 1; ww < NWV; ++ww) r = tmax(r, red[ww * 8 + q]);
        v[q] = r;
    }
}

// bounded spin on a device-scope counter (persistent mode only)
__device__ __forceinline__ bool grid_wait(unsigned int* ctr, const unsigned int target, int* status) {
    if (threadIdx.x == 0) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();     // 100 MHz
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(8);
            if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ULL) {    // 2 s: give up
                __hip_atomic_store(status + ST_TIMEOUT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __syncthreads();
    return true;
}

// ---------------------------------------------------------------------------
// symmetric-inverse path (lqp_spd.hpp): factorisation kernels
// ---------------------------------------------------------------------------
// standalone SPD inverse (test / utility entry lqp_spd_inverse_batched): dense (B,n,n) in, dense inverse out
template <int SEL = 1>          // 1: n <= 512 (wg_spd_sweep), 2: above (wg_spd_sweep_big): one sweep per instance, as k_spd_inverse
__global__ __launch_bounds__(LQP_NT) void k_spd_inverse_dense(const float* __restrict__ Kin, float* __restrict__ out,
                                                              float* __restrict__ Hs_all, int* __restrict__ info,
                                                              const int n, const int Ks, float* __restrict__ Yg_all) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    float* Hs = Hs_all + (size_t)b * sym_blocks(Ks) * LQP_BLK;
    if (tid == 0) info[b] = 0;
    wg_sym_init(Hs, Kin + (size_t)b * n * n, n, n, Ks, 0.f);
    __syncthreads();
    if constexpr (SEL == 2) wg_spd_sweep_big(Hs, Ks, info + b, smem, Yg_all + (size_t)b * (Ks - 1) * LQP_BLK);
    else wg_spd_sweep(Hs, Ks, info + b, smem);
    __syncthreads();
    float* o = out + (size_t)b * n * n;
    const int r = tid >> 4, c4 = (tid & 15) * 4;
    for (int j = 0; j < Ks; ++j)
        for (int i = j; i < Ks; ++i) {
            const V4<float> h = *(const V4<float>*)(Hs + (size_t)sym_idx(i, j, Ks) * LQP_BLK + tid * 4);
            const int gr = i * 64 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int gc = j * 64 + c4 + e;
                if (gr < n && gc < n) {
                    o[(size_t)gr * n + gc] = -h.v[e];
                    if (i != j) o[(size_t)gc * n + gr] = -h.v[e];
                }
            }
        }
}

// Si = S^-1 (S = Sm is symmetric positive definite, m <= 16: Gauss-Jordan without pivoting, Sm is destroyed): one thread per entry
// of [Sm | Si] -- 2 m^2 <= 512 of them -- and three barriers per column.  One thread used to walk through all of it: ~4 m^3
// dependent LDS round trips, ~0.25 ms per forward at m = 16 (inside the loop kernel's prologue).  The same operations on the same
// values per entry: the same bits.  Every thread of the workgroup calls; returns 1 when a pivot was not positive.
template <typename T, typename Barrier>
__device__ __forceinline__ int wg_gj_inverse_spd(T* __restrict__ Sm, T* __restrict__ Si, const int m, Barrier barrier) {
    const int tid = threadIdx.x, m2 = 2 * m;
    for (int i = tid; i < m * m; i += blockDim.x) Si[i] = (i / m == i % m) ? T(1) : T(0);
    const int rr = tid / m2, jj = tid - rr * m2;
    const bool mine = tid < m * m2;
    T* const ent = !mine ? Sm : (jj < m ? Sm + rr * m + jj : Si + rr * m + (jj - m));
    int bad = 0;
    barrier();
    for (int c = 0; c < m; ++c) {
        const T d = Sm[c * m + c];
        const T f = mine ? Sm[rr * m + c] : T(0);
        T* const pivot_row = jj < m ? Sm + c * m + jj : Si + c * m + (jj - m);
        if (!(d > T(0))) bad = 1;
        const T inv = d > T(0) ? T(1) / d : T(0);
        barrier();
        if (mine && rr == c) *ent *= inv;
        barrier();
        if (mine && rr != c) *ent -= f * *pivot_row;
        barrier();
    }
    return bad;
}

// equality rows: G = K^-1 A^T, S = A G, T = G S^-1, c = T b, s0 = S^-1 b, Hs += T G^T  (m <= SPD_MAXM)
// LDS: v | ylds | part[NW][Nps] | G[m][Nps] | Tl[m][Nps] | Sm[m*m] | Si[m*m]
__host__ __device__ inline int eqc_lds_bytes(int m, int Ks) {
    const int Nps = Ks * LQP_NB;
    return (Nps + sym_blocks(Ks) * 64 + LQP_NW * Nps + 2 * m * Nps + 2 * m * m + 8) * 4;
}
__device__ __forceinline__ void wg_eq_correct(const FwdParams<float>& P, const int b, char* smem) {
    const int n = P.n, m = P.m, Ks = P.Ks, Nps = Ks * LQP_NB;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float* v = (float*)smem;
    float* ylds = v + Nps;
    float* part = ylds + sym_blocks(Ks) * 64;
    float* G = part + (size_t)LQP_NW * Nps;
    float* Tl = G + (size_t)m * Nps;
    float* Sm = Tl + (size_t)m * Nps;
    float* Si = Sm + m * m;
    VecView<float> V(P.vecs + (size_t)b * P.vstride, n, m);
    float* Hs = P.packed + (size_t)b * packed_blocks(P.K) * LQP_BLK;
    BlockStream<float, LQP_NT> st;
    SymResident rr;
    // ---- G[q] = K^-1 a_q = -(Hs a_q) ----
    for (int q = 0; q < m; ++q) {
        for (int i = tid; i < Nps; i += LQP_NT) v[i] = i < n ? V.As[(size_t)q * n + i] : 0.f;
        __syncthreads();
        wg_sym_gemv<false>(st, rr, nullptr, 0, Hs, Ks, Nps, v, ylds, part);
        __syncthreads();
        for (int e = tid; e < Nps; e += LQP_NT) G[(size_t)q * Nps + e] = -sym_combine(e, Ks, Nps, ylds, part);
        __syncthreads();
    }
    // ---- S = A G (m x m), one wave per entry ----
    for (int t = w; t < m * m; t += LQP_NW) {
        const int q = t / m, q2 = t - q * m;
        float acc = 0.f;
        for (int i = lane; i < n; i += 64) acc += V.As[(size_t)q * n + i] * G[(size_t)q2 * Nps + i];
        acc = wave_sum(acc);
        if (lane == 0) Sm[t] = acc;
    }
    __syncthreads();
    // ---- S^-1 by Gauss-Jordan (S is SPD: no pivoting), m <= 16 ----
    {
        const int bad = wg_gj_inverse_spd(Sm, Si, m, [] { __syncthreads(); });
        if (bad && tid == 0) { if (P.info[b] == 0) P.info[b] = P.Ks * 64 + 1; P.status[ST_NOTSPD] = 1; }   // A rank deficient: not this path
    }
    __syncthreads();
    // ---- T = G S^-1, c = T b, s0 = S^-1 b ----
    for (int t = tid; t < m * Nps; t += LQP_NT) {
        const int q = t / Nps, e = t - q * Nps;
        float acc = 0.f;
        for (int q2 = 0; q2 < m; ++q2) acc += G[(size_t)q2 * Nps + e] * Si[q2 * m + q];
        Tl[t] = acc;
        if (e < n) V.Tm[(size_t)q * n + e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < n; e += LQP_NT) {
        float acc = 0.f;
        for (int q = 0; q < m; ++q) acc += Tl[(size_t)q * Nps + e] * V.bs[q];
        V.cv[e] = acc;
    }
    for (int q = tid; q < m; q += LQP_NT) {
        float acc = 0.f;
        for (int q2 = 0; q2 < m; ++q2) acc += Si[q * m + q2] * V.bs[q2];
        V.s0[q] = acc;
    }
    // ---- Hs += T G^T on every lower block (8 blocks' loads in flight at a time: one after the other the
    //      36 load -> update -> store round trips were pure latency) ----
    const int r = tid >> 4, c4 = (tid & 15) * 4;
    const int S = sym_blocks(Ks);
    int bi = 0, bj = 0;                                      // block (bi, bj) of stream position s0
    for (int s0 = 0; s0 < S; s0 += 8) {
        V4<float> h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (s0 + u < S) h[u] = *(const V4<float>*)(Hs + (size_t)(s0 + u) * LQP_BLK + tid * 4);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 + u < S) {
                for (int q = 0; q < m; ++q) {
                    const float t = Tl[(size_t)q * Nps + bi * 64 + r];
                    const V4<float> g = *(const V4<float>*)(G + (size_t)q * Nps + bj * 64 + c4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[u].v[e] += t * g.v[e];
                }
                *(V4<float>*)(Hs + (size_t)(s0 + u) * LQP_BLK + tid * 4) = h[u];
                if (++bi == Ks) { ++bj; bi = bj; }
            }
        }
    }
}

// (re)factorisation of the symmetric path for problem b: Hs = -(Qs + rho I)^-1, then the equality correction.
// check_sym: also verify that Qs is symmetric to rounding (the sweep only ever reads its lower triangle); a
// matrix that is not goes to the LU path like one that is not positive definite.
// SEL: 0 = any size (the continuation kernel's in-kernel refactorisation), 1 = n <= 512 only, 2 = above only: one sweep per
// instance of k_spd_inverse -- with both inlined the register allocator spilled 236 registers
template <int SEL = 0>
__device__ __forceinline__ void wg_spd_factor(const FwdParams<float>& P, const int b, const float rho, char* smem,
                                              const bool check_sym) {
    float* Hs = P.packed + (size_t)b * packed_blocks(P.K) * LQP_BLK;
    const bool lazy = P.scale && P.qs_lazy;
    const float* Qs = (P.scale && !lazy) ? (P.Qs + (size_t)b * P.n * P.ldq) : (P.Q + (size_t)b * P.n * P.n);
    const int ldq = (P.scale && !lazy) ? P.ldq : P.n;
    const float* dsc = lazy ? VecView<float>(P.vecs + (size_t)b * P.vstride, P.n, P.m).D : nullptr;
    if (check_sym && P.prep_fused && P.Ks <= SPD_MAXK) {
        // First factorisation behind k_spd_prep (the one-workgroup tier: more problems than half the CUs).  The UNSCALED
        // lower blocks are in the packed area already and the symmetry verdict went to the setup kernel: what is left is
        // element-wise -- (D_r v) D_c (the operations of sym_scale4: the same bits as the scaled copy), ||Qs||_F^2 on the way
        // (-> rho = clamp(||Qs||_F / sqrt(n)), :200-203, when rho is not given), rho on the diagonal.  Three passes over Q
        // less per solve (norm, symmetry check, block build: 0.6 of 7.9 ms at B = 1024, n = 500).
        const int n = P.n, Ks = P.Ks, tid = threadIdx.x, r = tid >> 4, c4 = (tid & 15) * 4;
        float* Dl = (float*)smem;                                    // [64 Ks] scaling vector, 1 on the padding
        float* red = Dl + 64 * Ks;
        for (int i = tid; i < 64 * Ks; i += LQP_NT) Dl[i] = i < n ? dsc[i] : 1.f;
        __syncthreads();
        const float* src = Hs + (size_t)(Ks & 1) * sym_blocks(Ks) * LQP_BLK;     // (where k_spd_prep leaves them: spd_half(P, b, Ks & 1))
        float fs = 0.f;
        for (int j = 0; j < Ks; ++j)
            for (int i = j; i < Ks; ++i) {
                const size_t off = (size_t)sym_idx(i, j, Ks) * LQP_BLK + tid * 4;
                V4<float> v = *(const V4<float>*)(src + off);
                const int gr = i * 64 + r, gc = j * 64 + c4;
                const float dr = Dl[gr];
                float t2 = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v.v[e] = (dr * v.v[e]) * Dl[gc + e];
                    t2 += (gr < n && gc + e < n) ? v.v[e] * v.v[e] : 0.f;      // (the identity on the padding is left out)
                }
                fs += i == j ? t2 : 2.f * t2;
                *(V4<float>*)(Hs + off) = v;
            }
        float rho_here = rho;
        if (P.rho_mode == 0) {
            const float fro = sqrtf(wg_sum(fs, red));
            rho_here = fro / (float)sqrt((double)n);
            rho_here = tmin(tmax(rho_here, P.rho_min), P.rho_max);
            if (tid == 0) P.scal[(size_t)b * SC_WORDS + SC_RHO] = rho_here;
        }
        __syncthreads();
        for (int i = 0; i < Ks; ++i) {                               // rho on the diagonal (own elements: written above by this thread)
            const int gr = i * 64 + r;
            if (gr < n && r >= c4 && r < c4 + 4) Hs[(size_t)sym_idx(i, i, Ks) * LQP_BLK + tid * 4 + (r - c4)] += rho_here;
        }
        __syncthreads();
    } else {
        if (check_sym) {
            float* red = (float*)smem;
            const float asym = wg_sym_asymmetry(Qs, ldq, P.n, P.Ks, red, dsc);
            if (threadIdx.x == 0 && asym > 0.f) { P.info[b] = P.Ks * 64 + 2; P.status[ST_NOTSPD] = 1; }
            __syncthreads();
        }
        wg_sym_init(Hs, Qs, ldq, P.n, P.Ks, rho, dsc);
        __syncthreads();
    }
    // (one sweep for both ways in: the blocks are in place either way)
    if (SEL == 2 || (SEL == 0 && P.Ks > SPD_MAXK)) wg_spd_sweep_big(Hs, P.Ks, P.info + b, smem, P.M + (size_t)b * P.Np * P.Np);   // (M: unused on this path)
    else wg_spd_sweep(Hs, P.Ks, P.info + b, smem, P.dbg ? P.dbg + (size_t)b * 8 : nullptr);
    if (threadIdx.x == 0 && P.info[b] != 0) P.status[ST_NOTSPD] = 1;
    if (P.m > 0) {
        __syncthreads();
        wg_eq_correct(P, b, smem);
    }
}
__host__ __device__ inline int spd_factor_lds_bytes(int m, int Ks) {
    const int a = spd_lds_bytes(Ks > SPD_MAXK ? SPD_MAXK : Ks), c = m > 0 ? eqc_lds_bytes(m, Ks) : 0;
    return a > c ? a : c;
}
template <int SEL = 1>          // 1: n <= 512 (wg_spd_sweep), 2: 512 < n <= 1024 (wg_spd_sweep_big)
__global__ __launch_bounds__(LQP_NT) void k_spd_inverse(const FwdParams<float> P, const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    const int b = blockIdx.x;
    wg_spd_factor<SEL>(P, b, P.scal[(size_t)b * SC_WORDS + SC_RHO], smem, gate == nullptr);
}

// ---- the same factorisation spread over launches: with fewer problems than half the CUs, SPD_NP workgroups share
//      one matrix.  begin (symmetry check, Qs + rho I -> blocks) | one launch per pivot step, out of place between
//      the two halves of the problem's packed area (K(K+1) >= 2 sym_blocks(Ks) blocks) | end (equality correction).
//      The parity of the first buffer is chosen so that the last step writes the half the loop reads. ----
constexpr int SPD_NP = 2;
__device__ __forceinline__ float* spd_half(const FwdParams<float>& P, const int b, const int which) {
    return P.packed + (size_t)b * packed_blocks(P.K) * LQP_BLK + (size_t)which * sym_blocks(P.Ks) * LQP_BLK;
}
template <int LQP_ANY = 0>      // (a template only so that the split build can place its one instance: tools/gen_split_build.py)
__global__ __launch_bounds__(LQP_NT) void k_spd_begin(const FwdParams<float> P, const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    int b, part;
    if (!shared_map((int)blockIdx.x, P.B, SPD_NP, b, part)) return;
    const bool lazy = P.scale && P.qs_lazy;
    const float* Qs = (P.scale && !lazy) ? (P.Qs + (size_t)b * P.n * P.ldq) : (P.Q + (size_t)b * P.n * P.n);
    const float* dsc = lazy ? VecView<float>(P.vecs + (size_t)b * P.vstride, P.n, P.m).D : nullptr;
    // rho_late (first factorisation only): this workgroup's share of ||Qs||_F^2 goes behind the sweep's exchange buffer,
    // the blocks are written without rho
    const bool late = gate == nullptr && P.rho_late;
    float* fro_out = late ? (P.M + (size_t)b * P.Np * P.Np + (size_t)2 * P.Ks * LQP_BLK + part) : nullptr;
    // (K <= 8: the launches after this one go back and forth between the two halves and end in half 0; above: in place)
    const float asym = wg_sym_check_init<SPD_NP>(spd_half(P, b, P.Ks > SPD_MAXK ? 0 : (P.Ks & 1)), Qs, (P.scale && !lazy) ? P.ldq : P.n, P.n, P.Ks,
                                                 late ? 0.f : P.scal[(size_t)b * SC_WORDS + SC_RHO], (float*)smem,
                                                 gate == nullptr, part, dsc, fro_out);
    if (threadIdx.x == 0 && asym > 0.f) { P.info[b] = P.Ks * 64 + 2; P.status[ST_NOTSPD] = 1; }
}
// Above 512 rows with rho = clamp(||Qs||_F / sqrt(n)) (FwdParams::rho_late): k_spd_begin has built the blocks WITHOUT rho and left
// the two workgroups' shares of ||Qs||_F^2 behind the panel area -- the setup kernel then makes one pass over Q (the column maxima)
// instead of two.  Here rho is formed (part 0 + part 1, the order fixed), stored, and added to the K diagonal tiles before the
// sweep's first launch reads them.
template <int LQP_ANY = 0>
__global__ __launch_bounds__(LQP_NT) void k_spd_rho_big(const FwdParams<float> P) {
    const int b = blockIdx.x, tid = threadIdx.x, n = P.n, Ks = P.Ks;
    const float* fr = P.M + (size_t)b * P.Np * P.Np + (size_t)2 * Ks * LQP_BLK;
    float rho = sqrtf(fr[0] + fr[1]) / (float)sqrt((double)n);
    rho = tmin(tmax(rho, P.rho_min), P.rho_max);
    if (tid == 0) P.scal[(size_t)b * SC_WORDS + SC_RHO] = rho;
    float* Hs = spd_half(P, b, 0);
    const int j = tid >> 6, t = tid & 63;
    if (j < Ks && j * 64 + t < n) Hs[(size_t)sym_idx(j, j, Ks) * LQP_BLK + t * 64 + t] += rho;
}
// the first factorisation's k_spd_begin, moved IN FRONT of the setup kernel (FwdParams::prep_fused): the column maxima the
// scaling starts from come out of the same pass over Q that checks its symmetry and builds the blocks -- unscaled; the
// resident sweep scales them as it loads them.  One pass over Q per solve instead of two.
static_assert(SPD_NP == 2, "k_fwd_setup reads the two halves k_spd_prep leaves");
template <int LQP_ANY = 0>      // (a template only so that the split build can place its one instance: tools/gen_split_build.py)
__global__ __launch_bounds__(LQP_NT) void k_spd_prep(const FwdParams<float> P) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    int b, part;
    if (!shared_map((int)blockIdx.x, P.B, SPD_NP, b, part)) return;
    float* sc = prep_scratch(P, b);
    const float asym = wg_sym_prep<SPD_NP>(spd_half(P, b, P.Ks & 1), P.Q + (size_t)b * P.n * P.n, P.n, P.n, P.Ks, (float*)smem,
                                           part, sc + (size_t)part * P.Ks * LQP_NB);
    if (threadIdx.x == 0) ((int*)(sc + (size_t)SPD_NP * P.Ks * LQP_NB))[part] = asym > 0.f ? 1 : 0;
}
template <int LQP_ANY = 0>      // (a template only so that the split build can place its one instance: tools/gen_split_build.py)
__global__ __launch_bounds__(LQP_NT) void k_spd_step(const FwdParams<float> P, const int* __restrict__ gate, const int k,
                                                      const int pivot_tasks) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    int b, part;                                                   // (the two workgroups of a matrix on one XCD: the panel is shared in its L2)
    if (!shared_map((int)blockIdx.x, P.B, SPD_NP, b, part)) return;
    // W, W^T of the next pivot block travel between the launches in the (unused on this path) KKT matrix area
    wg_spd_sweep<SPD_NP>(spd_half(P, b, (P.Ks - k) & 1), P.Ks, P.info + b, smem, nullptr, spd_half(P, b, (P.Ks - k - 1) & 1),
                         k, k + 1, part, P.M + (size_t)b * P.Np * P.Np, pivot_tasks);
}
// 512 < n <= 1024, few problems: one launch per PHASE of a pivot step (1: pivot block + Y phase, 2: tile updates), two
// workgroups per matrix, in place in half 0; the panel scratch is the (unused on this path) KKT matrix area.
template <int LQP_ANY = 0>      // (a template only so that the split build can place its one instance: tools/gen_split_build.py)
__global__ __launch_bounds__(LQP_NT) void k_spd_big_step(const FwdParams<float> P, const int* __restrict__ gate, const int k,
                                                          const int phases) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    int b, part;
    if (!shared_map((int)blockIdx.x, P.B, SPD_NP, b, part)) return;
    wg_spd_sweep_big<SPD_NP>(spd_half(P, b, 0), P.Ks, P.info + b, smem, P.M + (size_t)b * P.Np * P.Np, k, k + 1, phases, part);
}
// ---- what k_fwd_setup leaves to the resident sweep under prep_fused == 3 (the same operations on the same values as
//      there: the same bits).  d: the scaling vector in LDS. ----
// One wave each (they run beside the pivot block of the sweep's first step).
__device__ __forceinline__ void wave_deferred_vectors(const FwdParams<float>& P, const int b, const float* __restrict__ d) {
    const int n = P.n, lane = threadIdx.x & 63;
    VecView<float> V(P.vecs + (size_t)b * P.vstride, n, P.m);
    const float* p = P.p + (size_t)b * n;
    const float* lb = P.lb + (size_t)b * n;
    const float* ub = P.ub + (size_t)b * n;
    for (int i0 = 0; i0 < n; i0 += 256) {               // (twelve requests in flight)
        float pv[4], lv[4], uv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 64 * u + lane, ic = i < n ? i : n - 1;
            pv[u] = p[ic]; lv[u] = lb[ic]; uv[u] = ub[ic];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 64 * u + lane;
            if (i < n) {
                const float di = d[i];
                V.D[i] = di;
                V.ps[i] = di * pv[u];                // (:177)
                V.lbs[i] = lv[u] / di;               // (:192-194; +-inf / D stays +-inf)
                V.ubs[i] = uv[u] / di;
            }
        }
    }
}
// equality block: A D, row normalisation E (:179-190)
__device__ __forceinline__ void wave_deferred_eq_rows(const FwdParams<float>& P, const int b, const float* __restrict__ d) {
    const int n = P.n, m = P.m, lane = threadIdx.x & 63;
    if (m <= 0) return;
    VecView<float> V(P.vecs + (size_t)b * P.vstride, n, m);
    const float* A = P.A + (size_t)b * m * n;
    const float* bb = P.b + (size_t)b * m;
    float esum = 0.f, mine = 0.f;                           // lane r keeps the norm of row r (m <= SPD_MAXM <= 64)
    for (int r = 0; r < m; ++r) {
        float am = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float v = A[(size_t)r * n + j] * d[j];
            V.As[(size_t)r * n + j] = v;
            am = tmax(am, tabs(v));
        }
        am = wave_max(am);
        if (lane == r) mine = am;
        esum += am;
    }
    const float floor_a = tmax(esum / (float)m, 1e-6f);
    for (int r = 0; r < m; ++r) {
        float an = __shfl(mine, r);
        if (an <= 0.f) an = tmax(an, floor_a);
        const float e = 1.f / an;
        for (int j = lane; j < n; j += 64) V.As[(size_t)r * n + j] = e * V.As[(size_t)r * n + j];      // (this lane's own stores)
        if (lane == 0) { V.E[r] = e; V.bs[r] = e * bb[r]; }
    }
}
// the hooks of wg_spd_sweep_resident_v2 (RsNoScaling)
struct RsSetupHooks {
    const FwdParams<float>& P;
    int b, part, np;
    __device__ __forceinline__ void scaling(float* red, float* d, float* work) const {
        wg_scaling_vector<float, RS_NT>(P, b, red, 1, d, work, work + 8);
    }
    __device__ __forceinline__ void deferred(const float* d) const {
        if (part == 0) wave_deferred_vectors(P, b, d);
        if (part == np - 1) wave_deferred_eq_rows(P, b, d);
    }
};

// all pivot steps in ONE launch, the matrix resident in the registers of its two workgroups (lqp_spd.hpp).  Reads the
// blocks k_spd_begin built (half Ks & 1 of the packed area), leaves -(Qs + rho I)^-1 in half 0, where the loop reads it.
// Exchange buffer: the (unused on this path) KKT-matrix area; step flags: behind the loop's exchange granules.
template <int KS, int NP = 2, bool F16 = false>
__global__ __launch_bounds__(RS_NT) void k_spd_resident(const FwdParams<float> P, const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    int b, part;                                                   // (the NP workgroups of a problem on one XCD: shared_map)
    if (!shared_map((int)blockIdx.x, P.B, NP, b, part)) return;
    unsigned int* fl = (unsigned int*)(P.xchg + (size_t)P.B * XCHG_WORDS + (size_t)XCHG_TAIL * b);
    const unsigned int epoch = 32u * (unsigned int)P.status[ST_NFACTOR];
    RsLateRho lr;
    const bool fused = gate == nullptr && P.prep_fused;     // unscaled blocks from k_spd_prep (first factorisation only)
    const bool qpass = fused && P.prep_fused == 3;          // ... or no blocks at all: the sweep reads Q itself
    lr.on = (gate == nullptr && P.rho_late && !fused) ? 1 : 0;
    lr.n = P.n; lr.rho_min = P.rho_min; lr.rho_max = P.rho_max;
    lr.rho_out = part == 0 ? P.scal + (size_t)b * SC_WORDS + SC_RHO : nullptr;
    lr.dsc = (fused && !qpass) ? VecView<float>(P.vecs + (size_t)b * P.vstride, P.n, P.m).D : nullptr;
    lr.q = qpass ? P.Q + (size_t)b * P.n * P.n : nullptr;
    lr.cmx = qpass ? prep_scratch(P, b) : nullptr;
    lr.dbg_tid = 64 * (P.dbg_qpass >> 8);
    lr.piv_cols = P.piv_cols;
    lr.qdbg = (qpass && P.dbg && (P.dbg_qpass & 1) && part == 0) ? P.dbg + (size_t)(P.B + b) * 8 : nullptr;      // (LQP_DBG_QPASS=1: the debug buffer holds 2 B x 8 words)
    lr.fro_self = (fused && P.rho_mode == 0) ? 1 : 0;
    lr.rho_given = (fused && P.rho_mode != 0) ? P.scal[(size_t)b * SC_WORDS + SC_RHO] : 0.f;
    lr.xcd_local = P.xcd_local;
    const RsSetupHooks hooks{P, b, part, NP};
    wg_spd_sweep_resident_v2<KS, NP, RsSetupHooks, F16>(spd_half(P, b, KS & 1), spd_half(P, b, 0), P.M + (size_t)b * P.Np * P.Np, fl, epoch, part,
                                 P.info + b, P.status + ST_TIMEOUT, smem, lr,
                                 (P.dbg && part == 0) ? P.dbg + (size_t)b * 8 : nullptr, hooks);
}
template <int LQP_ANY = 0>      // (a template only so that the split build can place its one instance: tools/gen_split_build.py)
__global__ __launch_bounds__(LQP_NT) void k_spd_end(const FwdParams<float> P, const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    if (gate && *gate == 0) return;
    const int b = blockIdx.x;
    if (threadIdx.x == 0 && P.info[b] != 0) P.status[ST_NOTSPD] = 1;
    if (P.m > 0) wg_eq_correct(P, b, smem);
}

// equality duals of the last x-update.  LU path: the tail of the solve vector.  Symmetric path:
// nu = S^-1 (G^T w - b) = T^T w - s0, left in LDS by the loop
template <typename T, int NT, bool SYM>
__device__ __forceinline__ void loop_store_nu(const VecView<T>& V, const T* __restrict__ v, const T* __restrict__ nus_l,
                                              const int n, const int m) {
    const T* src = SYM ? nus_l : v + n;          // symmetric path: computed while v still held w (check / last iteration)
    for (int r = threadIdx.x; r < m; r += NT) V.nu[r] = src[r];
}
// LDS of the loop on the symmetric path; rl = LDS-resident blocks
__host__ __device__ inline int sym_loop_lds_bytes(int n, int m, int Ks, int rl, int nw = LQP_NW) {
    const int Nps = Ks * LQP_NB;
    return (rl * LQP_BLK + 3 * Nps + sym_blocks(Ks) * 64 + nw * Nps + 6 * n + 2 * m + nw * 8 + 8) * 4 + 64;
}
// how many blocks of the symmetric stream stay in LDS (after the LQP_RREG register blocks)
__host__ __device__ inline int sym_resident_lds_blocks(int n, int m, int Ks, int nreg = LQP_RREG, int nw = LQP_NW) {
    const int S = sym_blocks(Ks);
    int rl = S - nreg;
    if (rl < 0) rl = 0;
    while (rl > 0 && sym_loop_lds_bytes(n, m, Ks, rl, nw) > 160 * 1024) --rl;
    return rl;
}

// ---- epilogue: undo scaling, duals (:316-327), report ----
// Runs as the END of the forward's last kernel: k_fwd_epilogue, or the continuation loop kernel itself (`persistent & 4`:
// one launch and its boundary less per solve).  Also ORs the per-problem bound flags into the status block and, when the
// caller gave pinned host memory, reports there directly: every workgroup its own info / flag words, workgroup 0 the status
// block -- no device-to-host copy behind the solve (a 1.4 us blit kernel + a boundary).  Words other workgroups of the SAME
// launch may still write (ST_NOTSPD, ST_TIMEOUT of an in-kernel refactorisation) are therefore also kept per problem
// (RP_NOTSPD / RP_TIMEOUT in the writer's own flag word).
// With a separable term (fwd_finish<T, TERM>): the term's finish_elem at the returned iterate, its two outputs, and lams from u_box.
//
// ---------------------------------------------------------------------------
// The separable terms of the objective: sum_i f_i(x_i) beside the box, one trait each.  ADMM sees a term in ONE place, the z-update:
// z = clamp(prox_{f / rho}(x + u)) -- so a trait holds the element-wise prox and what surrounds it, and nothing else in the library
// knows a term: the scaled inputs k_term_setup leaves in the term's area of the workspace (FwdParams::termv: `slots` vectors of
// round_up(n, 8) per problem, the inputs first, then the thresholds = weights / rho that the streaming loop keeps for a launch), what
// a thread of a loop kernel holds per element (Regs), and what the epilogue reports for the backward (finish_elem: aux, u_box).
//   kind        FwdParams::term
//   input_flag  the bit of the problem's flag word that says "bad input" (setup_elem's verdict, OR-ed over the problem)
//   n_in        input vectors ([B][n] each, TermIn), slots: vectors of the area
//   Regs<T>     load: from the area with the rho of this launch (a division per element and launch, none per iteration); prox: the prox
//               at t = weight / rho, in the scaled space
//   View<T>     a pointer per vector of a problem's area -- the ONE place that states the area's layout; keep(i, rho) stores an element's
//               thresholds there (the streaming loop, TermOwn)
//   prox_at     (Regs) the prox of the thread's first element (registers) or of a further one (through the view)
//   setup_elem  one element of k_term_setup: scales the inputs into the area; true = this element's input is no input
//   finish_elem one element of the epilogue, in the scaled space where the kinks are exact
// Every prox returns v itself at a zero weight, by a branch: the plain step's bits.  A compile-time choice (Form*::term), never a flag.
// ---------------------------------------------------------------------------
constexpr int TERM_IN_MAX = 7;      // (the piecewise-linear term's four slopes and three kinks)
template <typename T> struct TermIn { const T* p[TERM_IN_MAX]; };
template <typename T> struct TermOut { T aux, u_box; };
template <typename TERM> __host__ __device__ inline size_t term_stride(int n) { return (size_t)TERM::slots * round_up(n, 8); }
struct TermNone {
    static constexpr int kind = 0, input_flag = 0, n_in = 0, slots = 0;
    template <typename T> struct Regs {
        __device__ __forceinline__ T prox(const T v) const { return v; }
    };
};
// L1 (lqp_boxqp_forward_l1), w |x - c|: soft-threshold around cs.  Area: [ws = D w | cs = c / D | t = ws / rho]
template <typename T> __device__ __forceinline__ T l1_shrink(const T v, const T t, const T c) {
    const T d = v - c;
    return d > t ? v - t : (d < -t ? v + t : c);
}
struct TermL1 {
    static constexpr int kind = 1, input_flag = RP_L1_INPUT, n_in = 2, slots = 3;
    enum { WS, CS, TH };
    template <typename T> struct View {
        T *ws = nullptr, *cs = nullptr, *t = nullptr;
        View() = default;
        __device__ __forceinline__ View(T* a, const int n) { ws = a + WS * round_up(n, 8); cs = a + CS * round_up(n, 8); t = a + TH * round_up(n, 8); }
        __device__ __forceinline__ void keep(const int i, const T rho) const { t[i] = ws[i] / rho; }
    };
    template <typename T> struct Regs {
        T t = T(0), c = T(0);
        __device__ __forceinline__ void load(const T* a, const int n, const int i, const T rho) { const View<const T> W(a, n); t = W.ws[i] / rho; c = W.cs[i]; }
        __device__ __forceinline__ T prox(const T v) const { return l1_shrink(v, t, c); }
        __device__ __forceinline__ T prox_at(const T v, const bool first, const View<T> W, const int i) const {
            return l1_shrink(v, first ? t : W.t[i], first ? c : W.cs[i]);
        }
    };
    // a weight that is negative or not finite: t = ws / rho would be no threshold
    template <typename T>
    static __device__ __forceinline__ bool setup_elem(T* a, const int n, const int i, const TermIn<T>& in, const size_t g, const T* D, const T*) {
        const View<T> W(a, n);
        const T wi = in.p[0][g], di = D[i];
        W.ws[i] = di * wi;
        W.cs[i] = in.p[1][g] / di;
        return !(wi >= T(0) && wi < T(INFINITY));            // (NaN fails the first comparison)
    }
    // The soft threshold once more at the returned iterate, in the scaled space where the kink is exact (z == cs by assignment):
    // v = z + u, S = l1_shrink(v, ws / rho, cs).  side = sign(S - cs), 0 exactly on the kink set (the threshold branch was taken and
    // t > 0); u_box = (S - clamp(S)) / D -- S - z with the clamp taken again, so that it is exactly zero unless the element is clamped
    // (the stored z is the clamp of the last iteration's v, one rounding away from this one) -- the box's share of the dual, and lams
    // are built from it; the rest of u is the L1 term's multiplier.
    template <typename T>
    static __device__ __forceinline__ TermOut<T> finish_elem(const T* a, const int n, const int i, const T zs, const T us, const T lbs,
                                                             const T ubs, const T d, const T rho, const T poison) {
        const View<const T> W(a, n);
        const T v = zs + us, t = W.ws[i] / rho, cs = W.cs[i], dd = v - cs;
        const bool kink = t > T(0) && !(dd > t) && !(dd < -t);
        const T S = l1_shrink(v, t, cs);
        const T ubx = (S - tmin(tmax(S, lbs), ubs)) / d + poison;      // (S - z with z = clamp(S): exactly zero off the bounds)
        return {(kink ? T(0) : (dd < T(0) ? T(-1) : T(1))) + poison, ubx};
    }
};
// Soft band (lqp_boxqp_forward_soft), wl (lo - x)_+ + wu (x - hi)_+: two thresholds tl = wls / rho, tu = wus / rho, two kinks
// los <= his; los == his with tl == tu is l1_shrink, bit for bit.  Area: [wls = D wl | wus = D wu | los = lo / D | his = hi / D | tl | tu]
template <typename T> __device__ __forceinline__ T soft_prox(const T v, const T tl, const T tu, const T los, const T his) {
    const T dh = v - his, dl = v - los;
    return dh > tu ? v - tu : (dl < -tl ? v + tl : tmin(tmax(v, los), his));
}
struct TermSoft {
    static constexpr int kind = 2, input_flag = RP_SOFT_INPUT, n_in = 4, slots = 6;
    enum { WLS, WUS, LOS, HIS, TL, TU };
    template <typename T> struct View {
        T *wls = nullptr, *wus = nullptr, *los = nullptr, *his = nullptr, *tl = nullptr, *tu = nullptr;
        View() = default;
        __device__ __forceinline__ View(T* a, const int n) {
            const int s = round_up(n, 8);
            wls = a + WLS * s; wus = a + WUS * s; los = a + LOS * s; his = a + HIS * s; tl = a + TL * s; tu = a + TU * s;
        }
        __device__ __forceinline__ void keep(const int i, const T rho) const { tl[i] = wls[i] / rho; tu[i] = wus[i] / rho; }
    };
    template <typename T> struct Regs {
        T tl = T(0), tu = T(0), lo = T(0), hi = T(0);
        __device__ __forceinline__ void load(const T* a, const int n, const int i, const T rho) {
            const View<const T> W(a, n);
            tl = W.wls[i] / rho; tu = W.wus[i] / rho; lo = W.los[i]; hi = W.his[i];
        }
        __device__ __forceinline__ T prox(const T v) const { return soft_prox(v, tl, tu, lo, hi); }
        __device__ __forceinline__ T prox_at(const T v, const bool first, const View<T> W, const int i) const {
            return first ? soft_prox(v, tl, tu, lo, hi) : soft_prox(v, W.tl[i], W.tu[i], W.los[i], W.his[i]);
        }
    };
    // a weight that is negative or not finite, lo > hi, a NaN in lo or hi (an infinite kink stays infinite)
    template <typename T>
    static __device__ __forceinline__ bool setup_elem(T* a, const int n, const int i, const TermIn<T>& in, const size_t g, const T* D, const T*) {
        const View<T> W(a, n);
        const T wli = in.p[0][g], wui = in.p[1][g], loi = in.p[2][g], hii = in.p[3][g], di = D[i];
        bool bad = !(wli >= T(0) && wli < T(INFINITY)) || !(wui >= T(0) && wui < T(INFINITY));      // (NaN fails the first comparison)
        bad |= !(loi <= hii);                                  // (lo > hi, or a NaN in either)
        W.wls[i] = di * wli;
        W.wus[i] = di * wui;
        W.los[i] = loi / di;
        W.his[i] = hii / di;
        return bad;
    }
    // The same with soft_prox; zone = +-2 on the sloped pieces, +-1 on the kinks hi / lo (only where the weight of that side is
    // positive: with none the kink is no kink), 0 inside the band; u_box as for L1.
    template <typename T>
    static __device__ __forceinline__ TermOut<T> finish_elem(const T* a, const int n, const int i, const T zs, const T us, const T lbs,
                                                             const T ubs, const T d, const T rho, const T poison) {
        const View<const T> W(a, n);
        const T v = zs + us, tl = W.wls[i] / rho, tu = W.wus[i] / rho, los = W.los[i], his = W.his[i];
        const T S = soft_prox(v, tl, tu, los, his);
        const T zone = (v - his > tu) ? T(2) : (v - los < -tl) ? T(-2) : (v >= his && tu > T(0)) ? T(1) : (v <= los && tl > T(0)) ? T(-1) : T(0);
        const T ubx = (S - tmin(tmax(S, lbs), ubs)) / d + poison;
        return {zone + poison, ubx};
    }
};
// Log barrier (lqp_boxqp_forward_log), -w log(x): the prox with t = w / rho is the positive root of S^2 - v S - t = 0.  With
// s = sqrt(v^2 + 4 t): 0.5 (v + s) for v >= 0 and 2 t / (s - v) for v < 0 -- the form without cancellation (0.5 (v + s) loses 5 % at
// v = -50, t = 1e-3 in float32).  Area: [ws = w | t = ws / rho] (in the scaled space x = D xs the term is -w log(xs) plus a constant:
// the weight takes no D)
template <typename T> __device__ __forceinline__ T log_prox(const T v, const T t) {
    if (t == T(0)) return v;
    const T s = tsqrt(v * v + T(4) * t);
    return v >= T(0) ? T(0.5) * (v + s) : (T(2) * t) / (s - v);
}
struct TermLog {
    static constexpr int kind = 3, input_flag = RP_LOG_INPUT, n_in = 1, slots = 2;
    enum { WS, TH };
    template <typename T> struct View {
        T *ws = nullptr, *t = nullptr;
        View() = default;
        __device__ __forceinline__ View(T* a, const int n) { ws = a + WS * round_up(n, 8); t = a + TH * round_up(n, 8); }
        __device__ __forceinline__ void keep(const int i, const T rho) const { t[i] = ws[i] / rho; }
    };
    template <typename T> struct Regs {
        T t = T(0);
        __device__ __forceinline__ void load(const T* a, const int n, const int i, const T rho) { t = View<const T>(a, n).ws[i] / rho; }
        __device__ __forceinline__ T prox(const T v) const { return log_prox(v, t); }
        __device__ __forceinline__ T prox_at(const T v, const bool first, const View<T> W, const int i) const { return log_prox(v, first ? t : W.t[i]); }
    };
    // a weight that is negative or not finite, or a barrier element whose upper bound is not positive (the domain is empty)
    template <typename T>
    static __device__ __forceinline__ bool setup_elem(T* a, const int n, const int i, const TermIn<T>& in, const size_t g, const T*, const T* ub) {
        const T wi = in.p[0][g];
        View<T>(a, n).ws[i] = wi;
        return !(wi >= T(0) && wi < T(INFINITY)) || (wi > T(0) && !(ub[g] > T(0)));      // (NaN fails the first comparison)
    }
    // At the returned iterate: u_box is the box's share of the dual, (us + t / zs) / D where the clamp moved S and exactly 0 elsewhere
    // (S - clamp(S) is NOT the multiplier here: the barrier's own force t / zs acts on a clamped element too); curv = w / z^2
    // (unscaled z) on the free barrier elements, the diagonal of the term's Hessian for the backward, 0 elsewhere.
    template <typename T>
    static __device__ __forceinline__ TermOut<T> finish_elem(const T* a, const int n, const int i, const T zs, const T us, const T lbs,
                                                             const T ubs, const T d, const T rho, const T poison) {
        const T wi = View<const T>(a, n).ws[i], t = wi / rho;
        const T S = log_prox(zs + us, t);
        const bool held = S != tmin(tmax(S, lbs), ubs);
        const T ubx = (held ? (t == T(0) ? us : us + t / zs) / d : T(0)) + poison;
        const T zu = d * zs;
        return {((wi > T(0) && !held) ? wi / (zu * zu) : T(0)) + poison, ubx};      // (curv)
    }
};
// Piecewise linear (lqp_boxqp_forward_pwl), f(x) = s_0 x + sum_k (s_k - s_{k-1}) (x - c_k)_+ with PWL_K sorted kinks and PWL_K + 1
// non-decreasing slopes: L1 (one kink, slopes -w, w), the band (two kinks, slopes -wl, 0, wu), both at once, tiered costs.  Fewer kinks are
// padded at the top: a kink at +inf and the last slope repeated.  Thresholds t_k = ss_k / rho; the prox scans from the top,
//   for k = K .. 1:  d = v - cs_k;  d > t_k: v - t_k;  d >= t_{k-1}: cs_k      and v - t_0 below the lowest kink
// -- these comparisons and no others: at slopes (-w, w, w, w) it is l1_shrink and at (-wl, 0, wu, wu) soft_prox, bit for bit (min_k
// max(v - t_k, cs_k) is the same number in exact arithmetic only).  Non-decreasing slopes that are zero at both ends are zero throughout:
// the branch of the plain step's bits looks at two.  Area: [cs_1 .. cs_K | ss_0 .. ss_K | t_0 .. t_K], cs_k = c_k / D, ss_k = D s_k
constexpr int PWL_K = 3;
template <typename T, typename TA, typename CA> __device__ __forceinline__ T pwl_prox(const T v, const TA& t, const CA& cs) {
    if (t[0] == T(0) && t[PWL_K] == T(0)) return v;
#pragma unroll
    for (int k = PWL_K; k >= 1; --k) {
        const T d = v - cs[k - 1];
        if (d > t[k]) return v - t[k];
        if (d >= t[k - 1]) return cs[k - 1];
    }
    return v - t[0];
}
struct TermPwl {
    static constexpr int K = PWL_K;
    static_assert(2 * K + 1 <= TERM_IN_MAX, "TermIn holds a pointer per slope and kink");
    // (n_in: the pointers of TermIn that cannot be null -- the K + 1 slopes and the first kink, then the further kinks, null = +inf)
    static constexpr int kind = 4, input_flag = RP_PWL_INPUT, n_in = K + 2, slots = 3 * K + 2;
    enum { CS = 0, SS = K, TH = 2 * K + 1 };
    template <typename T> struct View {
        T *cs[K] = {}, *ss[K + 1] = {}, *t[K + 1] = {};
        View() = default;
        __device__ __forceinline__ View(T* a, const int n) {
            const int s = round_up(n, 8);
#pragma unroll
            for (int k = 0; k < K; ++k) cs[k] = a + (CS + k) * s;
#pragma unroll
            for (int k = 0; k <= K; ++k) { ss[k] = a + (SS + k) * s; t[k] = a + (TH + k) * s; }
        }
        __device__ __forceinline__ void keep(const int i, const T rho) const {
#pragma unroll
            for (int k = 0; k <= K; ++k) t[k][i] = ss[k][i] / rho;
        }
    };
    template <typename T> struct Regs {
        T t[K + 1] = {}, c[K] = {};
        __device__ __forceinline__ void load(const T* a, const int n, const int i, const T rho) {
            const View<const T> W(a, n);
#pragma unroll
            for (int k = 0; k <= K; ++k) t[k] = W.ss[k][i] / rho;
#pragma unroll
            for (int k = 0; k < K; ++k) c[k] = W.cs[k][i];
        }
        __device__ __forceinline__ T prox(const T v) const { return pwl_prox(v, t, c); }
        __device__ __forceinline__ T prox_at(const T v, const bool first, const View<T> W, const int i) const {
            if (first) return pwl_prox(v, t, c);
            Regs o;
#pragma unroll
            for (int k = 0; k <= K; ++k) o.t[k] = W.t[k][i];
#pragma unroll
            for (int k = 0; k < K; ++k) o.c[k] = W.cs[k][i];
            return pwl_prox(v, o.t, o.c);
        }
    };
    // a slope that is not finite, slopes or kinks that decrease, a NaN kink (an infinite kink stays infinite; a null kink vector is +inf)
    template <typename T>
    static __device__ __forceinline__ bool setup_elem(T* a, const int n, const int i, const TermIn<T>& in, const size_t g, const T* D, const T*) {
        const View<T> W(a, n);
        const T di = D[i];
        bool bad = false;
        T prev = T(0);
#pragma unroll
        for (int k = 0; k <= K; ++k) {
            const T sk = in.p[k][g];
            bad |= !(sk > T(-INFINITY) && sk < T(INFINITY));        // (NaN fails the first comparison)
            if (k > 0) bad |= !(sk >= prev);
            prev = sk;
            W.ss[k][i] = di * sk;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T ck = in.p[K + 1 + k] ? in.p[K + 1 + k][g] : T(INFINITY);
            bad |= k > 0 ? !(ck >= prev) : !(ck == ck);            // (a NaN fails either)
            prev = ck;
            W.cs[k][i] = ck / di;
        }
        return bad;
    }
    // The scan once more at the returned iterate: piece = 2 k on the slope s_k, 2 k - 1 exactly on kink k -- only where its jump is
    // positive (t_k > t_{k-1}: with none the kink is no kink, and the element belongs to the piece below it, the band's tu > 0 rule);
    // u_box as for L1.
    template <typename T>
    static __device__ __forceinline__ TermOut<T> finish_elem(const T* a, const int n, const int i, const T zs, const T us, const T lbs,
                                                             const T ubs, const T d, const T rho, const T poison) {
        Regs<T> r;
        r.load(a, n, i, rho);
        const T v = zs + us;
        const T S = pwl_prox(v, r.t, r.c);
        int piece = 0;
#pragma unroll
        for (int k = K; k >= 1; --k) {
            const T dd = v - r.c[k - 1];
            if (dd > r.t[k]) { piece = 2 * k; break; }
            if (dd >= r.t[k - 1]) { piece = r.t[k] > r.t[k - 1] ? 2 * k - 1 : 2 * k - 2; break; }
        }
        const T ubx = (S - tmin(tmax(S, lbs), ubs)) / d + poison;
        return {T(piece) + poison, ubx};
    }
};
// Huber (lqp_boxqp_forward_huber), w H_delta(x - c) with H_delta(d) = 0.5 d^2 for |d| <= delta and delta |d| - 0.5 delta^2 beyond: the
// first term with zones AND curvature.  In the scaled space ws = D^2 w, cs = c / D, ds = delta / D.  With t = ws / rho the prox is
// v - t / (1 + t) (v - cs) where that lands inside the quadratic zone, |v - cs| <= ds (1 + t), and v -+ t ds beyond.  Per element and
// launch: q = t ds, lim = ds + q, sh = t / (1 + t); an iteration holds two compares and one multiply-subtract.  sh == 0 exactly where
// t == 0 (t >= 0), so the branch of the plain step's bits needs no register for t -- and it comes first: delta = +inf (lim = q = +inf, the
// quadratic branch always: a weighted least-squares term) makes q = 0 * inf a NaN at t == 0.  delta = 0 is no term (q = 0).
// Area: [ws | cs | ds | q | lim | sh]
template <typename T> __device__ __forceinline__ T huber_prox(const T v, const T c, const T q, const T lim, const T sh) {
    if (sh == T(0)) return v;
    const T d = v - c;
    return d > lim ? v - q : (d < -lim ? v + q : v - sh * d);
}
struct TermHuber {
    static constexpr int kind = 5, input_flag = RP_HUBER_INPUT, n_in = 3, slots = 6;
    enum { WS, CS, DS, QS, LIM, SH };
    template <typename T> struct View {
        T *ws = nullptr, *cs = nullptr, *ds = nullptr, *q = nullptr, *lim = nullptr, *sh = nullptr;
        View() = default;
        __device__ __forceinline__ View(T* a, const int n) {
            const int s = round_up(n, 8);
            ws = a + WS * s; cs = a + CS * s; ds = a + DS * s; q = a + QS * s; lim = a + LIM * s; sh = a + SH * s;
        }
        __device__ __forceinline__ void keep(const int i, const T rho) const {
            const T t = ws[i] / rho, qi = t * ds[i];
            q[i] = qi; lim[i] = ds[i] + qi; sh[i] = t / (T(1) + t);
        }
    };
    template <typename T> struct Regs {
        T c = T(0), q = T(0), lim = T(0), sh = T(0);
        __device__ __forceinline__ void load(const T* a, const int n, const int i, const T rho) {
            const View<const T> W(a, n);
            const T t = W.ws[i] / rho, dsi = W.ds[i];
            c = W.cs[i]; q = t * dsi; lim = dsi + q; sh = t / (T(1) + t);
        }
        __device__ __forceinline__ T prox(const T v) const { return huber_prox(v, c, q, lim, sh); }
        __device__ __forceinline__ T prox_at(const T v, const bool first, const View<T> W, const int i) const {
            return first ? huber_prox(v, c, q, lim, sh) : huber_prox(v, W.cs[i], W.q[i], W.lim[i], W.sh[i]);
        }
    };
    // a weight that is negative or not finite, a delta that is negative or NaN (+inf is the pure quadratic), a centre that is not finite
    template <typename T>
    static __device__ __forceinline__ bool setup_elem(T* a, const int n, const int i, const TermIn<T>& in, const size_t g, const T* D, const T*) {
        const View<T> W(a, n);
        const T wi = in.p[0][g], ci = in.p[1][g], dli = in.p[2][g], di = D[i];
        W.ws[i] = di * (di * wi);
        W.cs[i] = ci / di;
        W.ds[i] = dli / di;
        return !(wi >= T(0) && wi < T(INFINITY)) || !(dli >= T(0)) || !(ci > T(-INFINITY) && ci < T(INFINITY));      // (NaN fails the first comparison of each)
    }
    // The step's comparisons once more at the returned iterate (v = zs + us): zone = +-1 on the linear pieces, 0 on the quadratic zone
    // and wherever w = 0.  u_box as for the log barrier: the term's own force t clip(zs - cs, -ds, ds) acts on a clamped element too, so
    // the box's share of the dual is (us - that) / D where the clamp moved S, and exactly 0 elsewhere.
    template <typename T>
    static __device__ __forceinline__ TermOut<T> finish_elem(const T* a, const int n, const int i, const T zs, const T us, const T lbs,
                                                             const T ubs, const T d, const T rho, const T poison) {
        Regs<T> r;
        r.load(a, n, i, rho);
        const View<const T> W(a, n);
        const T v = zs + us, dd = v - r.c, t = W.ws[i] / rho, dsi = W.ds[i];
        const T S = huber_prox(v, r.c, r.q, r.lim, r.sh);
        const T zone = t == T(0) ? T(0) : dd > r.lim ? T(1) : dd < -r.lim ? T(-1) : T(0);
        const bool held = S != tmin(tmax(S, lbs), ubs);
        const T ubx = (held ? (t == T(0) ? us : us - t * tmin(tmax(zs - r.c, -dsi), dsi)) / d : T(0)) + poison;
        return {zone + poison, ubx};
    }
};
// What a thread of the streaming loop, which owns several elements, keeps of a term: its first element in registers; the thresholds
// of its further elements (n > NT only) come from the area, where prime() stores them itself -- nothing is stored for the first
// (both workgroups of a shared problem would write the same values).  Nothing at all for TermNone.
template <typename T, typename TERM> struct TermOwn {
    typename TERM::template Regs<T> r0;
    typename TERM::template View<T> W;
    template <int NT> __device__ __forceinline__ void prime(T* a, const int n, const int tid, const T rho) {
        W = typename TERM::template View<T>(a, n);
        for (int i = tid + NT; i < n; i += NT) W.keep(i, rho);
        if (tid < n) r0.load(a, n, tid, rho);
    }
    __device__ __forceinline__ T prox(const T v, const int i, const int tid) const { return r0.prox_at(v, i == tid, W, i); }
};
// (an empty specialisation, not dead members: with the members the plain instances of the streaming loop were no longer the
//  instructions they had been)
template <typename T> struct TermOwn<T, TermNone> {
    template <int NT> __device__ __forceinline__ void prime(T*, int, int, T) {}
    __device__ __forceinline__ T prox(const T v, int, int) const { return v; }
};

// lams = (max(-y, 0), max(y, 0)) of element e of problem b from y = rho * (the box's share of u) (:316-327)
template <typename T, typename I> __device__ __forceinline__ void lams_from_y(T* lams, const size_t b, const int n, const I e, const T y) {
    lams[b * 2 * n + e] = (-y > T(0)) ? -y : T(0);
    lams[b * 2 * n + n + e] = (y > T(0)) ? y : T(0);
}
template <typename T, typename TERM = TermNone>
__device__ __forceinline__ void fwd_finish(const FwdParams<T>& P, const int b, T* __restrict__ term_aux = nullptr, T* __restrict__ term_ubox = nullptr) {
    const int n = P.n, m = P.m, tid = threadIdx.x, nt = blockDim.x;
    VecView<T> V(P.vecs + (size_t)b * P.vstride, n, m);
    const T rho = P.scal[(size_t)b * SC_WORDS + SC_RHO];
    // a failed factorisation (singular KKT matrix / Q + rho I not positive definite) or a barrier timeout must not
    // leave plausible-looking numbers behind: callers that did not wait for the status see NaN
    const int info_b = P.info[b];
    const int notspd = __hip_atomic_load(P.status + ST_NOTSPD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int tmo = __hip_atomic_load(P.status + ST_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool bad = info_b != 0 || notspd != 0 || tmo != 0;
    if constexpr (TERM::kind != 0) bad = bad || (P.bflags[b] & TERM::input_flag) != 0;
    const T poison = bad ? T(__builtin_nanf("")) : T(0);
    for (int i = tid; i < n; i += nt) {
        const T d = V.D[i];
        const T xo = d * V.x[i] + poison, zo = d * V.z[i] + poison, uo = V.u[i] / d + poison;
        P.x[(size_t)b * n + i] = xo;
        P.z[(size_t)b * n + i] = zo;
        P.u[(size_t)b * n + i] = uo;
        T y = uo * rho;
        if constexpr (TERM::kind != 0) {
            const TermOut<T> o = TERM::finish_elem(P.termv + (size_t)b * term_stride<TERM>(n), n, i, V.z[i], V.u[i], V.lbs[i], V.ubs[i], d, rho, poison);
            term_aux[(size_t)b * n + i] = o.aux;
            term_ubox[(size_t)b * n + i] = o.u_box;
            y = o.u_box * rho;
        }
        lams_from_y(P.lams, (size_t)b, n, i, y);
    }
    for (int r = tid; r < m; r += nt) P.nus[(size_t)b * m + r] = V.nu[r] * V.E[r] + poison;
    if (tid == 0) P.rho_out[b] = rho;
    const int mine = P.bflags[b] | (tmo ? RP_TIMEOUT : 0) | ((notspd && P.spd && info_b != 0) ? RP_NOTSPD : 0);
    if (P.host_report && tid == 0) {
        __hip_atomic_store(P.host_report + ST_WORDS + b, info_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(P.host_report + ST_WORDS + P.B + b, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (b == 0) {
        // the bound flags of the batch (the per-problem words were written by an earlier launch)
        int f = 0;
        for (int i = tid; i < P.B; i += nt) f |= P.bflags[i];
        const int any_lb = __syncthreads_or(f & RP_LB) ? 1 : 0, any_ub = __syncthreads_or(f & RP_UB) ? 1 : 0;
        if (tid < ST_WORDS) {
            int v = __hip_atomic_load(P.status + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tid == ST_ANY_LB) v = (any_lb || (P.bound_flags_in && P.bound_flags_in[0] != 0)) ? 1 : 0;
            if (tid == ST_ANY_UB) v = (any_ub || (P.bound_flags_in && P.bound_flags_in[1] != 0)) ? 1 : 0;
            if (tid == ST_ANY_LB || tid == ST_ANY_UB) P.status[tid] = v;
            if (P.host_report) __hip_atomic_store(P.host_report + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// ---------------------------------------------------------------------------
// The steps an ADMM loop kernel is composed from (this file, lqp_loop_small.hpp, lqp_loop_split.hpp, lqp_dense.hpp): the
// element-wise update, the stopping check and its record, the blocking verdict and the stop record of stop = 'each'.
// Stateless; what differs between the kernels -- who owns which element, who reports, how many arrive -- is an argument.
// (Which kernel uses which step, and why some keep their own lines: DESIGN.md section 10.)
// ---------------------------------------------------------------------------
// The over-relaxed iterate xh = alpha x + (1 - alpha) z_prev (control['alpha'], OSQP's relaxation; alpha_c = 1 - alpha from the host).
// alpha == 1, the reference: x itself, bit for bit, and nothing between x and z but one scalar BRANCH on the uniform flag P.relax.  As
// a select, the factor, its mask and the wait for z_prev sat on the path from x to z in every iteration of the plain step (2.5 % of
// the split loop's time); the empty statement keeps the compiler from turning the branch back into one.
template <typename T>
__device__ __forceinline__ T admm_relax(const T xi, const T zp, const FwdParams<T>& P) {
    T xh = xi;
    if (P.relax) {
        asm volatile("");
        xh = P.alpha * xi + P.alpha_c * zp;
    }
    return xh;
}
// z-update, residuals and dual of one element (:271-282).  The projection and the dual see xh; the primal residual of the
// check stays x - z (the unrelaxed x, as in OSQP); at alpha == 1, xh - zn is r
template <typename T> struct AdmmStep { T zn, r, s, un; };
// With a separable term (TERM, `tr`: the element's thresholds) its prox stands between xh + u and the clamp; TermNone's is v itself
template <bool RELAX, typename TERM, typename T>
__device__ __forceinline__ AdmmStep<T> admm_step_term_as(const FwdParams<T>& P, const T xi, const T zp, const T ui, const T lb, const T ub,
                                                         const T rho, const typename TERM::template Regs<T> tr) {
    const T xh = RELAX ? P.alpha * xi + P.alpha_c * zp : xi;
    T zn = tr.prox(xh + ui);
    zn = tmin(tmax(zn, lb), ub);                             // (:273-276; an infinite bound is a no-op)
    const T r = xi - zn;
    return {zn, r, rho * (zn - zp), ui + (xh - zn)};
}
// ... for a kernel that decides on P.relax outside its iteration (k_admm_loop_split: one hot loop per value, so that the plain step's
// loop is the code it was): the step as a tag -- plain, relaxed, or a run-time branch on the uniform flag (see admm_relax)
struct RelaxOff { static constexpr int kind = 0; };
struct RelaxOn { static constexpr int kind = 1; };
struct RelaxDyn { static constexpr int kind = 2; };
template <typename TAG, typename TERM, typename T>
__device__ __forceinline__ AdmmStep<T> admm_step_term_tag(const FwdParams<T>& P, const T xi, const T zp, const T ui, const T lb, const T ub,
                                                          const T rho, const typename TERM::template Regs<T> tr) {
    if constexpr (TAG::kind == 2) {
        if (P.relax) {
            asm volatile("");
            return admm_step_term_as<true, TERM>(P, xi, zp, ui, lb, ub, rho, tr);
        }
        return admm_step_term_as<false, TERM>(P, xi, zp, ui, lb, ub, rho, tr);
    } else {
        return admm_step_term_as<TAG::kind == 1, TERM>(P, xi, zp, ui, lb, ub, rho, tr);
    }
}
// the plain step of a kernel without forms (lqp_dense.hpp)
template <typename T>
__device__ __forceinline__ AdmmStep<T> admm_step(const FwdParams<T>& P, const T xi, const T zp, const T ui, const T lb, const T ub,
                                                 const T rho) {
    return admm_step_term_tag<RelaxDyn, TermNone>(P, xi, zp, ui, lb, ub, rho, {});
}
// The FORM of a loop kernel: the ways a solve runs its loop, one tag each -- every loop family (admm_loop_body, admm_loop_small_body,
// admm_loop_split_body) has an instance per form it supports, named by the tag (k_admm_loop<..., lqp::FormEach>), and the host's
// LoopForm / by_form (lqp_amd.hip) is the run-time twin.  A combination that is no form cannot be written.
//   each:   control['stop'] = 'each' -- every problem stops and adapts rho as a batch of one
//   detect: ... with the primal infeasibility certificate at every check (control['infeasible'])
//   dual:   ... and the dual certificate beside it (control['unbounded'])
//   term:   the separable term whose prox the element-wise step takes (lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber); the batch stops as one
struct FormAll     { static constexpr bool each = false, detect = false, dual = false; using term = TermNone; };
struct FormEach    { static constexpr bool each = true,  detect = false, dual = false; using term = TermNone; };
struct FormDetect  { static constexpr bool each = true,  detect = true,  dual = false; using term = TermNone; };
struct FormCertify { static constexpr bool each = true,  detect = true,  dual = true;  using term = TermNone; };
struct FormL1      { static constexpr bool each = false, detect = false, dual = false; using term = TermL1; };
struct FormSoft    { static constexpr bool each = false, detect = false, dual = false; using term = TermSoft; };
struct FormLog     { static constexpr bool each = false, detect = false, dual = false; using term = TermLog; };
struct FormPwl     { static constexpr bool each = false, detect = false, dual = false; using term = TermPwl; };
struct FormHuber   { static constexpr bool each = false, detect = false, dual = false; using term = TermHuber; };
// ... and its terms of the six inf-norms of a check (:285-299).  qx = (Qs x)_i: the x-update solved (Qs + rho I) x + As^T nu = w
// exactly (to the solve's rounding), so Qs x = w - rho x - As^T nu without touching Q -- it only feeds a tolerance SCALE; the
// caller forms it from wherever its w, As and nu live.  ACC: the thread owns several elements (fold) or one (assign).
template <bool ACC, typename T>
__device__ __forceinline__ void admm_step_norms(T (&mx)[6], const AdmmStep<T>& st, const T xi, const T di, const T rho, const T qx) {
    const T nm[6] = {tabs(di * st.r), tabs(di * st.s), tabs(di * xi), tabs(di * st.zn), tabs((rho * di) * st.un), tabs(qx / di)};
#pragma unroll
    for (int q = 0; q < 6; ++q) mx[q] = ACC ? tmax(mx[q], nm[q]) : nm[q];
}
// The stopping check (:285-313) from the six norms of a problem: is it optimal, does it want another rho (:239-245), and the
// ratio for that step.  The ONE decision that fixes every iteration count and every adaptive-rho event.
template <typename T> struct LoopCheck { T ratio; bool solved, wants, trig; };
template <typename T>
__device__ __forceinline__ LoopCheck<T> loop_check(const FwdParams<T>& P, const T (&mv)[6], const T pnorm) {
    const T tiny = T(1e-16);
    const T pri_scale = tmax(tmax(mv[2], mv[3]), tiny);
    const T tol_p = P.eps_abs + P.eps_rel * pri_scale;
    const T dua_scale = tmax(tmax(tmax(mv[4], mv[5]), pnorm), tiny);
    const T tol_d = P.eps_abs + P.eps_rel * dua_scale;
    const bool solved = (mv[0] < tol_p) && (mv[1] < tol_d);
    const bool wants = (mv[0] > tmax(tol_p, P.ar_thr)) || (mv[1] > tmax(tol_d, P.ar_thr));
    const T num = tmax(mv[0] / pri_scale, tiny);
    const T den = tmax(mv[1] / dua_scale, tiny);
    const T ratio = tsqrt(num / den);
    const bool trig = (ratio > P.ar_tol) || (ratio < P.ar_inv_tol);
    return {ratio, solved, wants, trig};
}
// the check's record (one thread of the reporting workgroup): the problem's scalars -- SC_PRI / SC_DUA: primal / dual error of this
// check (the NumPy twin returns them); SC_TRIG: stop = 'each' only, where the problem decides its own rho event -- and the trace
template <bool EACH, typename T>
__device__ __forceinline__ void loop_check_store(const FwdParams<T>& P, T* scal, const LoopCheck<T>& ck, const T (&mv)[6],
                                                 const int it) {
    scal[SC_RATIO] = ck.ratio;
    scal[SC_WANTS] = ck.wants ? T(1) : T(0);
    if constexpr (EACH) scal[SC_TRIG] = ck.trig ? T(1) : T(0);
    scal[SC_PRI] = mv[0];
    scal[SC_DUA] = mv[1];
    trace_check(P.vtrace, it, P.check_solved, P.ring, mv[0], mv[1]);
}
// The blocking verdict (all workgroups resident): device-wide "all optimal?" (torch.all at :312) once `arrivals` workgroups have
// arrived.  True: the loop ends at iteration `it` (or a wait timed out); `writer` -- one thread of the grid -- says so.
template <typename T>
__device__ __forceinline__ bool loop_all_optimal(const FwdParams<T>& P, unsigned int* ct, const unsigned int arrivals, const int it,
                                                 const bool writer) {
    grid_wait(ct + CT_ARRIVE, arrivals, P.status);
    const unsigned int notopt = __hip_atomic_load(ct + CT_NOTOPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int tmo = __hip_atomic_load(P.status + ST_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (notopt != 0 && !tmo) return false;
    if (writer) {
        P.status[ST_FINAL_ITER] = it;
        __hip_atomic_store(P.status + ST_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return true;
}
// stop = 'each': problem b stopped at iteration `it` (one thread, after the iterate was stored).  The batch's final iteration is the
// largest; the count of stopped problems goes behind the RETURNED maximum, and whoever makes it B has therefore seen every maximum
// land before it raises ST_DONE
// why = 1: optimal; 2: flagged primal infeasible (control['infeasible']) -- also bit RP_INFEAS of the problem's flag word, which the
// forward's last kernel reports as it stands; 3: flagged dual infeasible (control['unbounded']), bit RP_UNBOUNDED
template <typename T>
__device__ __forceinline__ void each_stop(const FwdParams<T>& P, const int b, const int it, const int why = 1) {
    int* ps_ = P.pstat + (size_t)b * PS_WORDS;
    ps_[PS_FINAL] = it;
    ps_[PS_DONE] = why;
    if (why == 2) P.bflags[b] |= RP_INFEAS;
    if (why == 3) P.bflags[b] |= RP_UNBOUNDED;
    const int r1 = atomicMax(P.status + ST_FINAL_ITER, it);
    asm volatile("s_waitcnt vmcnt(0)" :: "v"(r1) : "memory");
    const int nd = __hip_atomic_fetch_add(P.status + ST_NDONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (nd + 1 == P.B) __hip_atomic_store(P.status + ST_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ---- control['infeasible'] (stop = 'each' only; P.snap != null): the primal infeasibility certificate at a check ----
// OSQP's test with the differences taken check to check, in the scaled problem: y = rho u, g = Qs x + s, nu of THIS check against the
// snapshot of the last one -- dy, dg, dnu; N = |dy|_inf; c1 = |dg|_inf / N; c2 = (sum_i [ubs_i max(dy_i, 0) + lbs_i min(dy_i, 0)] +
// bs^T dnu) / N.  Infeasible iff N > 0, c1 <= eps and c2 <= -eps: dy + As^T dnu = -dg by the x-update's stationarity, so (dy, dnu) is a
// Farkas certificate of {As x = bs, lbs <= x <= ubs} = empty.  An infinite bound: its term counts 0 while |dy_i| <= eps N, else c2 = +inf
// (0 * inf is never formed).  The snapshot is valid iff it is the last check's and rho has not changed since (an adaptive-rho event
// of this problem changes y's scale: the check behind it only refreshes).  Composed like the other steps: infeas_view (which slots,
// valid?), infeas_elem per element the caller owns, infeas_nu per equality row, infeas_decide on the four reduced numbers
// {N, |dg|_inf, largest |dy_i| on an infinite bound, the sum}, infeas_mark by one thread.  All of it on check iterations only.
template <typename T> struct InfeasView { const T* prev; T* next; int n; bool valid; int xo; };      // xo: where a slot's x lies, 0 = no dual certificate
template <typename T>
__device__ __forceinline__ InfeasView<T> infeas_view(const FwdParams<T>& P, const int b, const int it, const T rho) {
    T* base = P.snap + (size_t)b * P.snap_stride;
    const size_t len = P.snap_stride / 2;
    const int c = it / P.check_solved;
    const T* prev = base + (size_t)((c + 1) & 1) * len;
    const bool valid = it >= P.check_solved && prev[SN_MARK] == T(it - P.check_solved + 1) && prev[SN_RHO] == rho;
    return {prev, base + (size_t)(c & 1) * len, P.n, valid, P.eps_dinf > T(0) ? SN_HEAD + 2 * P.n + P.m : 0};
}
template <typename T>
__device__ __forceinline__ void infeas_elem(T (&ia)[4], const InfeasView<T>& S, const int i, const T y, const T g, const T lb,
                                            const T ub) {
    // (the other slot is read whether or not it is valid: the loads then do not wait for the slot's head, a memory round trip less on
    //  the check's path; what an invalid slot holds -- inside the region, whatever it is -- is dropped)
    const T py = S.prev[SN_HEAD + i], pg = S.prev[SN_HEAD + S.n + i];
    S.next[SN_HEAD + i] = y;
    S.next[SN_HEAD + S.n + i] = g;
    if (S.valid) {
        const T dy = y - py, dg = g - pg;
        ia[0] = tmax(ia[0], tabs(dy));
        ia[1] = tmax(ia[1], tabs(dg));
        const T bnd = dy > T(0) ? ub : lb;
        if (dy != T(0)) {
            if (tabs(bnd) <= std::numeric_limits<T>::max()) ia[3] += bnd * dy;
            else ia[2] = tmax(ia[2], tabs(dy));
        }
    }
}
template <typename T>
__device__ __forceinline__ void infeas_nu(T (&ia)[4], const InfeasView<T>& S, const int r, const T nu, const T bsr) {
    const T pnu = S.prev[SN_HEAD + 2 * S.n + r];
    S.next[SN_HEAD + 2 * S.n + r] = nu;
    if (S.valid) ia[3] += bsr * (nu - pnu);
}
template <typename T>
__device__ __forceinline__ void infeas_mark(const InfeasView<T>& S, const int it, const T rho) {
    S.next[SN_RHO] = rho;
    S.next[SN_MARK] = T(it + 1);
}
template <typename T>
__device__ __forceinline__ bool infeas_decide(const FwdParams<T>& P, const InfeasView<T>& S, const T (&iv)[4]) {
    if (!S.valid || !(P.eps_pinf > T(0))) return false;
    const T N = iv[0];
    if (!(N > T(0))) return false;
    if (iv[2] > P.eps_pinf * N) return false;                 // (c2 = +inf)
    return iv[1] / N <= P.eps_pinf && iv[3] / N <= -P.eps_pinf;
}
// ---- control['unbounded'] (P.eps_dinf > 0; S.xo != 0): the dual infeasibility certificate at the same check, on the same snapshot ----
// dx = x - x_prev, dq = Qs x - Qs x_prev (qx as the check forms it, from the right-hand side); N = |dx|_inf, e1 = |dq|_inf / N,
// e2 = ps^T dx / N, e3 = max_i([lbs_i finite] (-dx_i), [ubs_i finite] dx_i, 0) / N.  Dual infeasible iff N > 0, e1 <= eps, e2 <= -eps and
// e3 <= eps: dx has Qs dx = 0 and ps^T dx < 0 and lies in the recession cone of the box.  As dx is not tested: the x-update solves the
// equality-constrained system, As x = bs at every iteration.  da: {N, |dq|_inf, cone violation, ps^T dx} -- {max, max, max,
// sum} like the primal four.  Without the dual certificate neither array is loaded or stored.
template <typename T>
__device__ __forceinline__ void dinf_elem(T (&da)[4], const InfeasView<T>& S, const int i, const T x, const T qx, const T psi,
                                          const T lb, const T ub) {
    if (S.xo) {
        const T px = S.prev[S.xo + i], pq = S.prev[S.xo + S.n + i];
        S.next[S.xo + i] = x;
        S.next[S.xo + S.n + i] = qx;
        if (S.valid) {
            const T dx = x - px;
            da[0] = tmax(da[0], tabs(dx));
            da[1] = tmax(da[1], tabs(qx - pq));
            if (tabs(lb) <= std::numeric_limits<T>::max()) da[2] = tmax(da[2], -dx);
            if (tabs(ub) <= std::numeric_limits<T>::max()) da[2] = tmax(da[2], dx);
            da[3] += psi * dx;
        }
    }
}
template <typename T>
__device__ __forceinline__ bool dinf_decide(const FwdParams<T>& P, const InfeasView<T>& S, const T (&dv)[4]) {
    if (!S.valid || !S.xo) return false;
    const T N = dv[0];
    if (!(N > T(0))) return false;
    return dv[1] / N <= P.eps_dinf && dv[3] / N <= -P.eps_dinf && dv[2] / N <= P.eps_dinf;
}
// {max, max, max, sum} over the workgroup (NWV waves; red: NWV * 8 + 8 words, as wg_max_n), the same numbers in every thread; `dual`
// (uniform): the dual certificate's four ride in the same pair of barriers, words 4 .. 7 of a wave's eight
template <typename T, int NWV>
__device__ __forceinline__ void infeas_reduce(T (&ia)[4], T (&da)[4], const bool dual, T* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 3; ++q) ia[q] = wave_max(ia[q]);
    ia[3] = wave_sum(ia[3]);
    if (dual) {
#pragma unroll
        for (int q = 0; q < 3; ++q) da[q] = wave_max(da[q]);
        da[3] = wave_sum(da[3]);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[w * 8 + q] = ia[q];
        if (dual) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[w * 8 + 4 + q] = da[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        T r = red[q];
#pragma unroll 1
        for (int ww = 1; ww < NWV; ++ww) r = q < 3 ? tmax(r, red[ww * 8 + q]) : r + red[ww * 8 + q];
        ia[q] = r;
    }
    if (dual) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            T r = red[4 + q];
#pragma unroll 1
            for (int ww = 1; ww < NWV; ++ww) r = q < 3 ? tmax(r, red[ww * 8 + 4 + q]) : r + red[ww * 8 + 4 + q];
            da[q] = r;
        }
    }
}
// the rest of the step behind the element pass (every thread of the workgroup, uniform): equality rows, reduction, decision, mark.
// nus / bs: the duals of this check and the scaled right-hand side, wherever the caller holds them.  -> 0 neither, 2 primal infeasible
// (tested first), 3 dual infeasible: each_stop's `why`
template <typename T, int NT>
// dual (uniform; a constant in the DETECT / CERTIFY instances, S.xo != 0 in the split loop): the dual certificate's four numbers too
__device__ __forceinline__ int infeas_finish(const FwdParams<T>& P, const InfeasView<T>& S, T (&ia)[4], T (&da)[4], const bool dual,
                                             const T* nus, const T* bs, const int it, const T rho, T* red) {
    for (int r = threadIdx.x; r < P.m; r += NT) infeas_nu(ia, S, r, nus[r], bs[r]);
    infeas_reduce<T, NT / 64>(ia, da, dual, red);
    if (threadIdx.x == 0) infeas_mark(S, it, rho);
    if (infeas_decide(P, S, ia)) return 2;
    return dual && dinf_decide(P, S, da) ? 3 : 0;
}
// ---------------------------------------------------------------------------
// The ADMM loop (:235-313).  RES: resident head of the factor stream (registers + LDS); SYM: symmetric-inverse
// x-update instead of the cached triangular solves; NT: threads.
// TAIL = continuation launch of the speculative (no host sync) schedule.  It has its own name in traces /
// profiles, exits at once when the first launch converged and, when `persistent & 2`, does the adaptive-rho
// steps (:237-256) in-kernel: global decision from the counters of the last check, masked rho update and
// refactorisation by this workgroup -- LU path: at its first iteration (LU + re-pack); symmetric path: at every
// event inside [it0, it1), segment by segment.  Only this cold variant carries the factorisation code; the first
// (hot) launch stays lean.
// ---------------------------------------------------------------------------
// NP == 2 (symmetric path above 512 rows, first launch, 2 B workgroups resident: k_admm_loop_np2): workgroups `part` = 0 / 1 of a
// problem stream one RANGE of whole block columns of H each -- [0, jc) and [jc, Ks), about half of the blocks: twice the registers
// and LDS under the same matrix, half the stream per CU -- and exchange their partial products every iteration as tagged 8-byte
// granules (the hand-off of k_admm_loop_split: two buffers by iteration parity, tag = iteration + 1, the area zeroed by the setup
// kernel), added in the fixed order part 0 + part 1: both hold bit-identical iterates and run the element-wise update and the
// checks redundantly; part 0 alone reports to the counters and writes state.
//
// EACH (control['stop'] = 'each', NP == 1 only): every problem is solved as the reference would solve it in a batch of one.  It
// stops at the first check at which IT is optimal (its workgroup stores the iterate, marks pstat[b] and returns), it adapts rho at
// an event iff its own `wants && trig` of the last check say so, and nothing crosses workgroups: no grid_wait, no arrival word,
// no decision from the counters.  A launch begins by reading pstat[b].done and leaves at once when it is set.
template <typename T, bool RES, bool TAIL, int NT, bool SYM, int NP, typename FORM>
__device__ __forceinline__ void admm_loop_body_from(const FwdParams<T>& P, int it0, const int it1, int ctr_base, int prev_slot,
                                                    const int persistent, char* smem);
// does the adaptive-rho event at iteration seg0 change this problem's rho?  The reference's decision over the whole batch, from the
// counters of the last check (uniform over the grid) -- or, EACH, the problem's own
template <typename T, bool EACH>
__device__ __forceinline__ bool loop_event_fires(const FwdParams<T>& P, const T* __restrict__ scal, const int seg0) {
    if constexpr (EACH) {
        return scal[SC_WANTS] != T(0) && scal[SC_TRIG] != T(0);
    } else {
        unsigned int* ctl = P.counters + (size_t)(((seg0 - 1) / P.check_solved) % P.ring) * CT_WORDS;
        return __hip_atomic_load(ctl + CT_WANTS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0 &&
               __hip_atomic_load(ctl + CT_TRIG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0;      // uniform over the whole grid
    }
}
// ... and the bookkeeping of a refactorisation inside the continuation kernel.  EACH: n_factor counts an event iteration once, whoever
// of its problems refactorises first (a bit per event in the two spare vote words, which only the strict global stop uses; from the
// 65th event on every refactorisation counts) -- it moves whenever the host must look at the info words again
template <typename T, bool EACH>
__device__ __forceinline__ void loop_event_count(const FwdParams<T>& P, const int b, const int seg0 = 0) {
    if constexpr (EACH) {
        if (threadIdx.x == 0) {
            ++P.pstat[(size_t)b * PS_WORDS + PS_NFACTOR];
            const int ev = seg0 / P.ar_iter - 1;
            bool first = true;
            if (ev >= 0 && ev < 64) {
                const int bit = 1 << (ev & 31);
                first = (atomicOr(P.status + ST_VOTE + 2 + (ev >> 5), bit) & bit) == 0;
            }
            if (first) atomicAdd(P.status + ST_NFACTOR, 1);
            __hip_atomic_store(P.status + ST_RHO_UPDATED, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        if (b == 0 && threadIdx.x == 0) { P.status[ST_NFACTOR] += 1; P.status[ST_RHO_UPDATED] = 1; }
    }
}
// the masked rho update of an event that fires (:246-256): the new rho of problem b, stored and counted; the caller refactorises
template <typename T, bool EACH>
__device__ __forceinline__ T loop_event_rho(const FwdParams<T>& P, T* scal, const int b, const int seg0) {
    T rho_ = scal[SC_RHO];
    if (scal[SC_WANTS] != T(0)) rho_ = rho_ * scal[SC_RATIO];
    rho_ = tmin(tmax(rho_, P.rho_min), P.rho_max);
    __syncthreads();
    if (threadIdx.x == 0) scal[SC_RHO] = rho_;
    loop_event_count<T, EACH>(P, b, seg0);
    return rho_;
}
// FORM (FormAll ... FormLog), read as EACH, DETECT, DUAL, L1, SOFT and LOG below:
// DETECT (control['infeasible']): the certificate at every check (infeas_view ...), instances of their own: inside the one body
// its registers cost the plain EACH kernels 3 % of their time
// DUAL (control['unbounded']): the dual certificate too, instances of their own again (FormCertify): under a
// run-time flag its registers cost the primal-only DETECT kernels 3 % (6 % in the small loop) of their time
// FORM::term: the separable term of the element-wise step (TermOwn) -- the kernels of lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber are instances of their own
template <typename T, bool RES, bool TAIL, int NT, bool SYM, int NP, typename FORM>
__device__ __forceinline__ void admm_loop_body(const FwdParams<T>& P, const int it0, const int it1,
                                               const int ctr_base,       // counter slot of check it0 / check
                                               const int prev_slot,      // slot of the last check before it0, -1: none / known not done
                                               const int persistent, char* smem) {
    // every problem stopped at an earlier check -> nothing to do (break at :312)
    if (__hip_atomic_load(P.status + ST_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    if constexpr (FORM::each) {
        // this problem stopped in an earlier launch: its iterate is not touched again
        if (__builtin_amdgcn_readfirstlane(P.pstat[(size_t)blockIdx.x * PS_WORDS + PS_DONE])) return;
    }
    admm_loop_body_from<T, RES, TAIL, NT, SYM, NP, FORM>(P, it0, it1, ctr_base, prev_slot, persistent, smem);
}
template <typename T, bool RES, bool TAIL, int NT, bool SYM, int NP, typename FORM>
__device__ __forceinline__ void admm_loop_body_from(const FwdParams<T>& P, int it0, const int it1, int ctr_base, int prev_slot,
                                                    const int persistent, char* smem) {
    static constexpr bool EACH = FORM::each, DETECT = FORM::detect, DUAL = FORM::dual;      // (static: never a lambda's capture)
    using TERM = typename FORM::term;
    static_assert(NP == 1 || (NP == 2 && SYM && RES && !TAIL && NT == 1024 && sizeof(T) == 4), "two workgroups per problem: the hot symmetric loop only");
    static_assert(!EACH || NP == 1, "per-problem stopping on the streaming loop: one workgroup per problem (the split loop has its own EACH form)");
    int b = blockIdx.x, part_id = 0;
    if constexpr (NP == 2) { if (!shared_map((int)blockIdx.x, P.B, 2, b, part_id)) return; }
    const bool lead = part_id == 0;                          // (the workgroup that reports and writes state)
    const int n = P.n, m = P.m, N = P.N, Np = P.Np, K = P.K;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if constexpr (TAIL) {
        // persistent & 8: the hot two-workgroup loop ran past the first possible rho event (FwdParams::hot_past) and names the
        // iteration at which it stopped -- an event that changes something, or the end of its range
        if (persistent & 8) {
            const int r = __builtin_amdgcn_readfirstlane(P.status[ST_RESUME]);
            if (r > 0) {
                it0 = r;
                ctr_base = ((r + P.check_solved - 1) / P.check_solved) % P.ring;
                prev_slot = ((r - 1) / P.check_solved) % P.ring;
            }
        }
    }
    if (!EACH && prev_slot >= 0) {        // (EACH: pstat[b].done and ST_DONE, read by admm_loop_body, say all there is to say)
        if (__hip_atomic_load(P.counters + (size_t)prev_slot * CT_WORDS + CT_NOTOPT, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) == 0) {
            if (b == 0 && tid == 0 && lead) {
                P.status[ST_FINAL_ITER] = it0 - 1;
                __hip_atomic_store(P.status + ST_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
    }
    if (it0 >= it1) return;
    // LDS carve.  LU path:  [resident blocks] v tmp | z u ps lb ub D bs red | dest
    //            SYM path: [resident blocks] v xs ylds cvl part[NW][Nps] | z u ps lb ub D bs red
    const int Nps = SYM ? P.Ks * LQP_NB : Np;                // padded length of the solve vector
    int rl = SYM ? (NT == 512 ? P.sym_rl_hot : P.sym_rl) : LQP_RLDS;
    // NP == 2: this workgroup's range of the stream -- block columns [rj0, rj0 + rwc), rsn blocks from stream index rs0.  Only ITS
    // row-sum slots and column sums are kept (the layout the host sized holds them for the whole stream): what that frees holds
    // more blocks of H -- three / two at Ks = 16.
    int rj0 = 0, rs0 = 0, rsn = -1, rwc = P.Ks;
    int ylds_slots = SYM ? sym_blocks(P.Ks) : 0, part_stride = Nps;
    if constexpr (NP == 2) {
        const int S_ = sym_blocks(P.Ks);
        int jc = 0, acc = 0;
        while (jc < P.Ks && 2 * acc < S_) { acc += P.Ks - jc; ++jc; }      // columns [0, jc): the first to reach half of the blocks
        rj0 = part_id == 0 ? 0 : jc; rs0 = part_id == 0 ? 0 : acc; rsn = part_id == 0 ? acc : S_ - acc;
        rwc = part_id == 0 ? jc : P.Ks - jc;
        const int freed = (S_ - rsn) * 64 + (NT / 64) * (Nps - rwc * 64);      // floats
        ylds_slots = rsn; part_stride = rwc * 64;
        rl += freed / LQP_BLK;
    }
    T* lds_res = (T*)smem;                                   // resident blocks (RES only), 16-KB aligned chunks
    T* v = lds_res + (RES ? (size_t)rl * LQP_BLK : 0);
    T* tmp = v + Nps;                                        // LU: 64 scratch; SYM: xs (the new x)
    T* xs = tmp;
    T* ylds = xs + Nps;                                      // SYM: one 64-slot per block of the stream
    T* cvl = ylds + (size_t)ylds_slots * 64;
    T* part = cvl + Nps;
    T* z = SYM ? part + (size_t)(NT / 64) * part_stride : tmp + 64;
    T* u = z + n;
    T* ps = u + n;
    T* lb = ps + n;
    T* ub = lb + n;
    T* D = ub + n;
    T* bs = D + n;
    T* red = bs + (SYM ? 2 * m : m);                        // SYM: nu of the current check sits behind bs
    int* dest = (int*)(red + (NT / 64) * 8 + 8);             // LU only

    VecView<T> V(P.vecs + (size_t)b * P.vstride, n, m);
    T* scal = P.scal + (size_t)b * SC_WORDS;
    const T* packed = P.packed + (size_t)b * packed_blocks(K) * LQP_BLK;
    // The continuation launch of the symmetric path walks through SEGMENTS [seg0, seg1) that end at the
    // adaptive-rho events (:237-256) and refactorises in between, inside the kernel; every other build runs
    // exactly one segment [it0, it1).
    int seg0 = it0;
    const int it_end = it1;
  while (true) {
    int seg1 = it_end;
    if constexpr (TAIL && SYM) {
        if (P.adaptive_rho && (persistent & 2)) {
            const int nxt = (seg0 / P.ar_iter + 1) * P.ar_iter;
            if (nxt < P.ar_max && nxt < seg1) seg1 = nxt;
            if (seg0 > 0 && seg0 % P.ar_iter == 0 && seg0 < P.ar_max) {
                if (loop_event_fires<T, EACH>(P, scal, seg0)) {
                    const T rho_ = loop_event_rho<T, EACH>(P, scal, b, seg0);
                    wg_spd_factor(P, b, rho_, smem, false);
                    __syncthreads();
                }
            }
        }
    }
    if constexpr (TAIL && !SYM && NT == 1024) {
        // The LU path's continuation launch walks through the adaptive-rho events (:237-256) the same way (round 5: one launch
        // per possible event before -- nine at the defaults, each ~5 us of nothing when the solve was over): the decision from the
        // counters of the last check (complete: every check of a persistent launch ends in a device-wide wait), the masked rho
        // update, KKT re-assembly, pivoted LU and pack in-kernel.
        if (P.adaptive_rho && (persistent & 2)) {
            const int nxt = (seg0 / P.ar_iter + 1) * P.ar_iter;
            if (nxt < P.ar_max && nxt < seg1) seg1 = nxt;
            if (seg0 > 0 && seg0 % P.ar_iter == 0 && seg0 < P.ar_max) {
                if (loop_event_fires<T, EACH>(P, scal, seg0)) {
                    constexpr int kPB = sizeof(T) == 4 ? 16 : 8;
                    const T rho_ = loop_event_rho<T, EACH>(P, scal, b, seg0);
                    const bool lazy_ = P.scale && P.qs_lazy;
                    const T* Qs_ = (P.scale && !lazy_) ? (P.Qs + (size_t)b * n * P.ldq) : (P.Q + (size_t)b * n * n);
                    assemble_kkt_rows(P, b, Qs_, (P.scale && !lazy_) ? P.ldq : n, V, rho_, true, lazy_ ? V.D : nullptr);
                    __syncthreads();
                    wg_lu_factor<T, kPB, sizeof(T) == 4, NT>(P.M + (size_t)b * Np * Np, N, Np, P.piv + (size_t)b * Np,
                                                                P.info + b, smem, nullptr);
                    __syncthreads();
                    wg_pack_factor<T>(P.M + (size_t)b * Np * Np, N, Np, P.piv + (size_t)b * Np,
                                      P.packed + (size_t)b * packed_blocks(K) * LQP_BLK, P.dest + (size_t)b * Np, smem, true);
                    __syncthreads();
                }
            }
        }
    }
    const int it0 = seg0, it1 = seg1;                        // (shadow the launch bounds inside the segment)
    const T rho = scal[SC_RHO];
    const T pnorm = scal[SC_PNORM];
    const int S = SYM ? sym_blocks(P.Ks) : K * (K + 1);
    const bool cyclic = true;                 // (wg_packed_solve pads the stream to a multiple of the ring depth)

    BlockStream<T, NT> st;
    ResidentRegs<T, NT> rr;
    const T* packed_r = packed + (size_t)rs0 * LQP_BLK;
    unsigned long long* const xq = NP == 2 ? P.xchg + (size_t)b * XCHG_WORDS : nullptr;
    // (LDS-resident blocks actually used: the layout is sized for the whole stream, a range may be shorter than registers + rl)
    int rl_use = rl;
    if constexpr (NP == 2) { const int room = rsn - resident_regs<NT>(); rl_use = room < 0 ? 0 : (room < rl ? room : rl); }
    if constexpr (SYM) {
        if constexpr (RES) {
            const int Sr_ = NP == 2 ? rsn : S;
            sym_resident_load<NT>(rr, lds_res, packed_r, Sr_, rl_use);
            sym_prime<NT>(st, packed_r, (Sr_ < resident_regs<NT>() ? Sr_ : resident_regs<NT>()) + rl_use, Sr_);
        }
    } else if constexpr (RES) {
        resident_load<T, NT>(rr, lds_res, packed);
        stream_prime_from<T, NT>(st, packed, resident_total<NT>(), S);
    } else {
        stream_prime<T, NT>(st, packed, S);
    }

    for (int i = tid; i < n; i += NT) {
        z[i] = V.z[i]; u[i] = V.u[i]; ps[i] = V.ps[i]; lb[i] = V.lbs[i]; ub[i] = V.ubs[i]; D[i] = V.D[i];
    }
    for (int r = tid; r < m; r += NT) bs[r] = V.bs[r];
    // the term's thresholds = weights / rho with this segment's rho (a division per element and rho, none per iteration)
    TermOwn<T, TERM> own;
    if constexpr (TERM::kind != 0) own.template prime<NT>(P.termv + (size_t)b * term_stride<TERM>(n), n, tid, rho);
    if constexpr (SYM) {
        for (int i = tid; i < Nps; i += NT) cvl[i] = (i < n && m > 0) ? V.cv[i] : T(0);
        if constexpr (NP == 2) {       // (every slot / column sum of the range is written by every product; zeroed once all the same)
            for (int i = tid; i < ylds_slots * 64; i += NT) ylds[i] = T(0);
            for (int i = tid; i < (NT / 64) * part_stride; i += NT) part[i] = T(0);
        }
    } else {
        const int* gdest = P.dest + (size_t)b * Np;
        for (int i = tid; i < Np; i += NT) dest[i] = gdest[i];
    }
    const T* xv = SYM ? xs : v;                              // where the x-update leaves x
    auto store_state = [&]() {                               // the iterate as it stands, for the next launch / the epilogue
        for (int i = tid; i < n; i += NT) { V.z[i] = z[i]; V.u[i] = u[i]; V.x[i] = xv[i]; }
        loop_store_nu<T, NT, SYM>(V, v, bs + m, n, m);
    };
    __syncthreads();

    unsigned long long dbt[4] = {0, 0, 0, 0}, dt0 = 0;      // debug: cycles in rhs / product / combine / update+check
    const bool dbg_on = SYM && P.dbg != nullptr;
    int slot = TAIL ? ((it0 + P.check_solved - 1) / P.check_solved) % P.ring : ctr_base;
    for (int it = it0; it < it1; ++it) {
        if (dbg_on) dt0 = clock64();
        const bool check = (it % P.check_solved) == 0;
        T mx[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) mx[q] = T(0);
        T ia[4] = {T(0), T(0), T(0), T(0)};                      // (DETECT: the certificate's terms, see infeas_view)
        T da[4] = {T(0), T(0), T(0), T(0)};                      // (... and the dual certificate's, see dinf_elem)
        InfeasView<T> isv = {nullptr, nullptr, n, false, 0};
        if constexpr (DETECT) { if (check) isv = infeas_view(P, b, it, rho); }
        // ||Q x / D||_inf of the check (:299) without touching Q: the x-update solved (Qs + rho I) x + As^T nu = w
        // exactly (to the solve's rounding), so Qs x = w - rho x - As^T nu.  It only feeds a tolerance SCALE.
        if constexpr (SYM) {
            // ---- symmetric path: product | barrier | ONE fused element-wise pass (combine, z/u update, residual
            //      norms, next right-hand side) | barrier.  v holds w = -p + rho (z - u) on entry. ----
            if (it == it0) {
                for (int i = tid; i < Nps; i += NT) v[i] = (i < n) ? -ps[i] + rho * (z[i] - u[i]) : T(0);
                wg_barrier_lds();
            }
            if (dbg_on) { const unsigned long long t = clock64(); dbt[0] += t - dt0; dt0 = t; }
            if constexpr (NP == 2)         // (the range's slots and column sums: base pointers moved so that the walk's own indices fit)
                wg_sym_gemv<RES, NT>(st, rr, lds_res, rl_use, packed_r, P.Ks, part_stride, v, ylds - (size_t)rs0 * 64, part - (size_t)rj0 * 64,
                                     rj0, rs0, rsn);
            else wg_sym_gemv<RES, NT>(st, rr, lds_res, rl, packed, P.Ks, Nps, v, ylds, part);
            wg_barrier_lds();
            if (dbg_on) { const unsigned long long t = clock64(); dbt[1] += t - dt0; dt0 = t; }
            T* nus_l = bs + m;
            if ((check || it + 1 == it1) && m > 0) {         // nu = T^T w - s0 (one wave per row) while v is still w
                for (int r = w; r < m; r += (NT / 64)) {
                    T acc = T(0);
                    for (int i = lane; i < n; i += 64) acc += V.Tm[(size_t)r * n + i] * v[i];
                    acc = wave_sum(acc);
                    if (lane == 0) nus_l[r] = acc - V.s0[r];
                }
                wg_barrier_lds();
            }
            if (dbg_on) { const unsigned long long t = clock64(); dbt[2] += t - dt0; dt0 = t; }
            for (int i = tid; i < Nps; i += NT) {
                T ysum;
                if constexpr (NP == 2) {
                    // the partial product of this workgroup's columns: row sums of the blocks (bi, j), j in its range, j <= bi; column sums
                    // where column bi is its own (the terms of sym_combine that are not zero for this range, in sym_combine's order)
                    const int bi = i >> 6, r_ = i & 63;
                    ysum = T(0);
                    const int jhi = bi < rj0 + rwc - 1 ? bi : rj0 + rwc - 1;
                    for (int j = rj0; j <= jhi; ++j) ysum += ylds[(size_t)(sym_idx(bi, j, P.Ks) - rs0) * 64 + r_];
                    if (bi >= rj0 && bi < rj0 + rwc) {
#pragma unroll
                        for (int ww = 0; ww < NT / 64; ++ww) ysum += part[(size_t)ww * part_stride + (i - rj0 * 64)];
                    }
                } else {
                    ysum = sym_combine<NT>(i, P.Ks, Nps, ylds, part);
                }
                if constexpr (NP == 2) {
                    // this workgroup's partial out, the partner's in (one granule per element, thread i = element i)
                    const unsigned int tag = (unsigned int)(it + 1);
                    unsigned long long* base = xq + (size_t)(it & 1) * (2 * SPD_BIGK * LQP_NB);
                    __hip_atomic_store(base + (size_t)part_id * (SPD_BIGK * LQP_NB) + i,
                                       ((unsigned long long)tag << 32) | (unsigned long long)__builtin_bit_cast(unsigned int, ysum),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long* src = base + (size_t)(1 - part_id) * (SPD_BIGK * LQP_NB) + i;
                    unsigned long long g = 0;
                    unsigned int spins = 0;
                    unsigned long long t0 = 0;
                    bool lost = false;
                    for (;;) {
                        g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((unsigned int)(g >> 32) == tag) break;
                        if ((++spins & 1023u) == 0) {
                            const unsigned long long now = __builtin_amdgcn_s_memrealtime();     // 100 MHz
                            if (t0 == 0) t0 = now;
                            else if (now - t0 > 50000000ULL ||
                                     __hip_atomic_load(P.status + ST_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {      // 0.5 s: give up, flagged
                                __hip_atomic_store(P.status + ST_TIMEOUT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                lost = true;
                                break;
                            }
                        }
                    }
                    // (a partner that never showed up must not leave plausible numbers: NaN from here on, and the time-out word)
                    const T other = lost ? T(__builtin_nanf("")) : __builtin_bit_cast(float, (unsigned int)g);
                    ysum = part_id == 0 ? ysum + other : other + ysum;
                }
                const T xi = cvl[i] - ysum;
                xs[i] = xi;
                T wn = T(0);
                if (i < n) {
                    const T zp = z[i];
                    const T ui = u[i];
                    const T xh = admm_relax(xi, zp, P);      // (the lines of admm_step)
                    T zn = xh + ui;
                    if constexpr (TERM::kind != 0) zn = own.prox(zn, i, tid);
                    zn = tmin(tmax(zn, lb[i]), ub[i]);     // (:273-276; an infinite bound is a no-op)
                    const T r = xi - zn;
                    const T s = rho * (zn - zp);
                    const T un = ui + (xh - zn);
                    z[i] = zn;
                    u[i] = un;
                    if (check) {
                        const T di = D[i];
                        mx[0] = tmax(mx[0], tabs(di * r));
                        mx[1] = tmax(mx[1], tabs(di * s));
                        mx[2] = tmax(mx[2], tabs(di * xi));
                        mx[3] = tmax(mx[3], tabs(di * zn));
                        mx[4] = tmax(mx[4], tabs((rho * di) * un));
                        T qx = v[i] - rho * xi;
                        for (int q = 0; q < m; ++q) qx -= V.As[(size_t)q * n + i] * nus_l[q];
                        mx[5] = tmax(mx[5], tabs(qx / di));
                        if constexpr (DETECT) { infeas_elem(ia, isv, i, rho * un, qx + s, lb[i], ub[i]); if constexpr (DUAL) dinf_elem(da, isv, i, xi, qx, ps[i], lb[i], ub[i]); }
                    }
                    wn = -ps[i] + rho * (zn - un);           // next iteration's right-hand side
                }
                v[i] = wn;
            }
        } else {
            // ---- rhs = [-p + rho (z - u); b], scattered to its pivoted position (:259-262) ----
            for (int i = tid; i < Np; i += NT) {
                T val = T(0);
                if (i < n) val = -ps[i] + rho * (z[i] - u[i]);
                else if (i < N) val = bs[i - n];
                v[dest[i]] = val;
            }
            wg_barrier_lds();
            // ---- x-update: cached triangular solves (:267) ----
            if constexpr (RES) {
                wg_packed_solve_resident<T, NT>(st, rr, lds_res, packed, K, v, tmp, true);
            } else {
                wg_packed_solve<T, NT>(st, packed, K, v, tmp, cyclic);
                if (!cyclic && it + 1 < it1) stream_prime<T, NT>(st, packed, S);
            }
            // ---- z-update, residuals, dual (:271-282) ----
            const T* nul = v + n;                            // nu is the tail of the solution
            for (int i = tid; i < n; i += NT) {
                const T xi = v[i];
                const T zp = z[i];
                const T ui = u[i];
                const T xh = admm_relax(xi, zp, P);          // (the lines of admm_step)
                T zn = xh + ui;
                if constexpr (TERM::kind != 0) zn = own.prox(zn, i, tid);
                zn = tmin(tmax(zn, lb[i]), ub[i]);
                const T r = xi - zn;
                const T s = rho * (zn - zp);
                const T un = ui + (xh - zn);
                z[i] = zn;
                u[i] = un;
                if (check) {
                    const T di = D[i];
                    mx[0] = tmax(mx[0], tabs(di * r));
                    mx[1] = tmax(mx[1], tabs(di * s));
                    mx[2] = tmax(mx[2], tabs(di * xi));
                    mx[3] = tmax(mx[3], tabs(di * zn));
                    mx[4] = tmax(mx[4], tabs((rho * di) * un));
                    T qx = -ps[i] + rho * (zp - ui) - rho * xi;
                    for (int q = 0; q < m; ++q) qx -= V.As[(size_t)q * n + i] * nul[q];
                    mx[5] = tmax(mx[5], tabs(qx / di));
                    if constexpr (DETECT) { infeas_elem(ia, isv, i, rho * un, qx + s, lb[i], ub[i]); if constexpr (DUAL) dinf_elem(da, isv, i, xi, qx, ps[i], lb[i], ub[i]); }
                }
            }
        }
        if (check) {
            T mv[6] = {mx[0], mx[1], mx[2], mx[3], mx[4], mx[5]};
            wg_max_n<T, 6, NT / 64>(mv, red);
            const T tiny = T(1e-16);
            const T pri_scale = tmax(tmax(mv[2], mv[3]), tiny);
            const T tol_p = P.eps_abs + P.eps_rel * pri_scale;
            const T dua_scale = tmax(tmax(tmax(mv[4], mv[5]), pnorm), tiny);
            const T tol_d = P.eps_abs + P.eps_rel * dua_scale;
            const bool solved = (mv[0] < tol_p) && (mv[1] < tol_d);
            const bool wants = (mv[0] > tmax(tol_p, P.ar_thr)) || (mv[1] > tmax(tol_d, P.ar_thr));
            // ratio for the next adaptive-rho step (:239-245)
            const T num = tmax(mv[0] / pri_scale, tiny);
            const T den = tmax(mv[1] / dua_scale, tiny);
            const T ratio = tsqrt(num / den);
            const bool trig = (ratio > P.ar_tol) || (ratio < P.ar_inv_tol);
            unsigned int* ct = P.counters + (size_t)slot * CT_WORDS;
            if constexpr (EACH) {
                if (tid == 0) {
                    scal[SC_RATIO] = ratio;
                    scal[SC_WANTS] = wants ? T(1) : T(0);
                    scal[SC_TRIG] = trig ? T(1) : T(0);
                    scal[SC_PRI] = mv[0];
                    scal[SC_DUA] = mv[1];
                    trace_check(P.vtrace, it, P.check_solved, P.ring, mv[0], mv[1]);
                    // a problem that is not optimal counts into its check's slot in every mode: k_check_done (the end of a host-driven
                    // chunk, persistent or per segment) reads it as it always has
                    if (!solved) atomicAdd(ct + CT_NOTOPT, 1u);
                }
                ++slot;
                int flagged = 0;                             // control['infeasible'] / ['unbounded']: 2 primal, 3 dual infeasible at this check (optimal comes first)
                if constexpr (DETECT) { flagged = infeas_finish<T, NT>(P, isv, ia, da, DUAL, SYM ? bs + m : v + n, bs, it, rho, red); if (solved) flagged = 0; }
                if (solved || flagged) {
                    // leave with the state of iteration `it`: the iterate first, then the words that say so
                    __syncthreads();
                    store_state();
                    if (tid == 0) {
                        each_stop(P, b, it, flagged ? flagged : 1);
                    }
                    return;
                }
            } else {
            if (tid == 0 && lead) {
                scal[SC_RATIO] = ratio;
                scal[SC_WANTS] = wants ? T(1) : T(0);
                scal[SC_PRI] = mv[0];                        // primal / dual error of this check (the NumPy twin returns them)
                scal[SC_DUA] = mv[1];
                trace_check(P.vtrace, it, P.check_solved, P.ring, mv[0], mv[1]);
                unsigned int r1 = 0, r2 = 0;
                if (wants) r1 = atomicAdd(ct + CT_WANTS, 1u);
                if (trig) r2 = atomicAdd(ct + CT_TRIG, 1u);
                if (persistent & 1) {
                    // the arrival and this problem's verdict in ONE 64-bit add (NOTOPT and ARRIVE share an aligned word), behind
                    // the RETURNED adds above: whoever sees the last arrival sees every counter of the check.  Nothing else
                    // is handed over here -- no release fence (an L2 write-back, microseconds per check)
                    asm volatile("s_waitcnt vmcnt(0)" :: "v"(r1), "v"(r2) : "memory");
                    __hip_atomic_fetch_add((unsigned long long*)(ct + CT_NOTOPT), (solved ? 0ull : 1ull) | (1ull << 32),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (!solved) {
                    atomicAdd(ct + CT_NOTOPT, 1u);
                }
            }
            ++slot;
            if (persistent & 1) {
                // all workgroups resident: device-wide "all optimal?" (torch.all at :312)
                grid_wait(ct + CT_ARRIVE, NP == 2 ? (unsigned int)P.B : gridDim.x, P.status);      // (one arrival per problem)
                const unsigned int notopt = __hip_atomic_load(ct + CT_NOTOPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int tmo = __hip_atomic_load(P.status + ST_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (notopt == 0 || tmo) {
                    if (b == 0 && tid == 0 && lead) {
                        P.status[ST_FINAL_ITER] = it;
                        __hip_atomic_store(P.status + ST_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    // leave the loop with the state of iteration `it`
                    __syncthreads();
                    if (lead) {
                        store_state();
                    }
                    if (dbg_on && tid == 0 && lead) {
                        dbt[3] += clock64() - dt0;
                        for (int q = 0; q < 4; ++q) P.dbg[(size_t)b * 8 + q] += dbt[q];
                    }
                    return;
                }
            }
            }       // (!EACH)
        }
        wg_barrier_lds();
        if (dbg_on) { const unsigned long long t = clock64(); dbt[3] += t - dt0; }
    }
    if (dbg_on && tid == 0 && lead)
        for (int q = 0; q < 4; ++q) P.dbg[(size_t)b * 8 + q] += dbt[q];
    // ---- save state for the next launch / the epilogue ----
    if (lead) {
        store_state();
    }
    if constexpr (EACH) {       // not optimal so far: the last iteration it ran (max_iters - 1 once the schedule is through)
        if (tid == 0) P.pstat[(size_t)b * PS_WORDS + PS_FINAL] = it1 - 1;
    }
    if (!TAIL || seg1 >= it_end) break;
    seg0 = seg1;
    __syncthreads();
  }
}
// the first launch of the symmetric path above 512 rows on TWO workgroups per problem (admm_loop_body_from, NP == 2): FormAll, FormL1, FormSoft, FormLog, FormPwl, FormHuber
template <typename FORM>
__global__ __launch_bounds__(1024) void k_admm_loop_np2(const FwdParams<float> P, const int it0, const int it1, const int ctr_base,
                                                        const int prev_slot, const int persistent) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    admm_loop_body<float, true, false, 1024, true, 2, FORM>(P, it0, it1, ctr_base, prev_slot, persistent, smem);
}

// The one-workgroup loop in every form.  persistent & 4 (continuation launches, FormAll): this is the forward's LAST launch -- it ends
// with the epilogue (fwd_finish).  No other form ever is the last launch: under stop = 'each' the workgroups leave at different times,
// and a term's epilogue takes two more outputs (k_fwd_epilogue<T, TERM>) -- a launch of its own for all.
template <typename T, bool RES, bool TAIL, int NT, bool SYM, typename FORM>
__global__ __launch_bounds__(NT) void k_admm_loop(const FwdParams<T> P, const int it0, const int it1, const int ctr_base,
                                                  const int prev_slot, const int persistent) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    admm_loop_body<T, RES, TAIL, NT, SYM, 1, FORM>(P, it0, it1, ctr_base, prev_slot, persistent, smem);
    if constexpr (TAIL && std::is_same<FORM, FormAll>::value) {
        if (persistent & 4) {
            __syncthreads();                   // (the state the loop left in global memory: written by other threads)
            fwd_finish(P, blockIdx.x);
        }
    }
}

// all problems optimal at the check held in `slot` (iteration `it_check`)?  -> DONE
template <int LQP_ANY = 0>      // (a template only so that the split build can place its one instance: tools/gen_split_build.py)
__global__ void k_check_done(int* status, const unsigned int* counters, const int slot, const int it_check) {
    if (threadIdx.x == 0 && status[ST_DONE] == 0 && counters[(size_t)slot * CT_WORDS + CT_NOTOPT] == 0) {
        status[ST_FINAL_ITER] = it_check;
        status[ST_DONE] = 1;
    }
}

// ---------------------------------------------------------------------------
// adaptive rho (:237-256): global decision from the counters of the last
// check, masked per-problem update, KKT re-assembly; sets the gate for the
// LU + pack launches that follow.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_rho_update(const FwdParams<T> P, int last_slot, const int max_it = 0) {
    const int b = blockIdx.x, n = P.n, m = P.m;
    if (__hip_atomic_load(P.status + ST_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (b == 0 && threadIdx.x == 0) P.status[ST_GATE] = 0;
        return;
    }
    if (last_slot < 0) {
        // the event iteration is where the hot loop stopped (FwdParams::hot_past): an event only if it left FOR one
        const int r = P.status[ST_RESUME];
        if (!(r > 0 && r % P.ar_iter == 0 && r < P.ar_max && r < max_it)) {
            if (b == 0 && threadIdx.x == 0) P.status[ST_GATE] = 0;
            return;
        }
        last_slot = ((r - 1) / P.check_solved) % P.ring;
    }
    bool fire, mine;
    T* scal = P.scal + (size_t)b * SC_WORDS;
    if (P.pstat) {
        // control['stop'] = 'each': a running problem adapts iff its own last check says so (:238, :244-246 over a batch of one);
        // the gate goes up when any does, and the chain then refactorises the whole batch -- a problem whose rho stays gets the
        // factor it had (the LU path re-assembles its matrix below: the factorisation is in place)
        int f = 0;
        for (int i = threadIdx.x; i < P.B; i += LQP_NT) {
            const T* si = P.scal + (size_t)i * SC_WORDS;
            f |= (P.pstat[(size_t)i * PS_WORDS + PS_DONE] == 0 && si[SC_WANTS] != T(0) && si[SC_TRIG] != T(0)) ? 1 : 0;
        }
        fire = __syncthreads_or(f) != 0;
        mine = P.pstat[(size_t)b * PS_WORDS + PS_DONE] == 0 && scal[SC_WANTS] != T(0) && scal[SC_TRIG] != T(0);
    } else {
        const unsigned int* ct = P.counters + (size_t)last_slot * CT_WORDS;
        const bool all_done = ct[CT_NOTOPT] == 0;
        fire = !all_done && ct[CT_WANTS] > 0 && ct[CT_TRIG] > 0;
        mine = scal[SC_WANTS] != T(0);
    }
    if (b == 0 && threadIdx.x == 0) {
        P.status[ST_GATE] = fire ? 1 : 0;
        if (fire) { P.status[ST_NFACTOR] += 1; P.status[ST_RHO_UPDATED] = 1; }
    }
    if (!fire) return;
    VecView<T> V(P.vecs + (size_t)b * P.vstride, n, m);
    T rho = scal[SC_RHO];
    if (mine) rho = rho * scal[SC_RATIO];
    // (stop = 'each': a problem that does not adapt keeps its rho to the bit -- the clamp is part of the update, :248-250)
    if (!P.pstat || mine) rho = tmin(tmax(rho, P.rho_min), P.rho_max);
    __syncthreads();
    if (threadIdx.x == 0) scal[SC_RHO] = rho;
    if (P.spd) return;
    const bool lazy = P.scale && P.qs_lazy;
    const T* Qs = (P.scale && !lazy) ? (P.Qs + (size_t)b * n * P.ldq) : (P.Q + (size_t)b * n * n);
    assemble_kkt_rows(P, b, Qs, (P.scale && !lazy) ? P.ldq : n, V, rho, true, lazy ? V.D : nullptr);
}

// primal / dual error of the last convergence check, per problem (lqp_boxqp_last_residuals)
// the check trace of a verbose solve (trace_check): bit patterns -> float32 in the caller's buffer
template <int LQP_ANY = 0>
__global__ void k_copy_trace(const unsigned int* __restrict__ vtrace, float* __restrict__ out, const int words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) out[i] = __uint_as_float(vtrace[i]);
}
// per-problem iteration counts of a control['stop'] = 'each' solve (lqp_boxqp_problem_iters)
template <int LQP_ANY = 0>
__global__ void k_copy_iters(const int* __restrict__ pstat, int* __restrict__ out, const int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = pstat[(size_t)b * PS_WORDS + PS_FINAL];
}
// how every problem of a control['stop'] = 'each' solve ended (lqp_boxqp_problem_status): 0 optimal, 1 out of iterations, 2 flagged
// primal infeasible, 3 flagged dual infeasible
template <int LQP_ANY = 0>
__global__ void k_copy_pstatus(const int* __restrict__ pstat, int* __restrict__ out, const int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        const int d = pstat[(size_t)b * PS_WORDS + PS_DONE];
        out[b] = d == 1 ? 0 : (d == 2 || d == 3 ? d : 1);
    }
}
// control['infeasible']: no problem has a snapshot yet -- the marks of both slots (infeas_view), at the head of every attempt
template <typename T>
__global__ void k_snap_init(T* __restrict__ snap, const size_t stride, const int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * B) snap[(size_t)(i >> 1) * stride + (size_t)(i & 1) * (stride / 2) + SN_MARK] = T(0);
}
template <typename T>
__global__ void k_copy_residuals(const T* __restrict__ scal, T* __restrict__ pri, T* __restrict__ dua, const int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        if (pri) pri[b] = scal[(size_t)b * SC_WORDS + SC_PRI];
        if (dua) dua[b] = scal[(size_t)b * SC_WORDS + SC_DUA];
    }
}

// ---------------------------------------------------------------------------
// epilogue: undo scaling, duals (:316-327)
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_fwd_epilogue(const FwdParams<T> P) {
    fwd_finish(P, blockIdx.x);
}
// ... of a solve with a separable term: the term's two outputs beside (an overload: the plain kernel keeps its name)
template <typename T, typename TERM>
__global__ __launch_bounds__(256) void k_fwd_epilogue(const FwdParams<T> P, T* __restrict__ aux, T* __restrict__ u_box) {
    fwd_finish<T, TERM>(P, blockIdx.x, aux, u_box);
}
// A solve with a separable term, behind the prologue (the scaling vector exists whichever kernel made it): the term's scaled inputs
// into its area, next to lbs / ubs' problem, and the input checks that need the data -- what the term's setup_elem refuses, or a rho
// of the problem (a per-problem rho_in among them) that is not positive and finite: weight / rho would be no threshold -- mark the
// problem (TERM::input_flag: NaN outputs, LQP_ERR_INVALID from whoever reads the report)
template <typename T, typename TERM>
__global__ __launch_bounds__(256) void k_term_setup(const FwdParams<T> P, const TermIn<T> in) {
    const int b = blockIdx.x, n = P.n, tid = threadIdx.x;
    VecView<T> V(P.vecs + (size_t)b * P.vstride, n, P.m);
    T* const area = P.termv + (size_t)b * term_stride<TERM>(n);
    const T rho = P.scal[(size_t)b * SC_WORDS + SC_RHO];
    bool bad = !(rho > T(0) && rho < T(INFINITY));
    for (int i = tid; i < n; i += 256) bad |= TERM::setup_elem(area, n, i, in, (size_t)b * n + i, V.D, P.ub);
    if (__syncthreads_or(bad ? 1 : 0) && tid == 0) P.bflags[b] |= TERM::input_flag;
}

// ---------------------------------------------------------------------------
// fixed-point backward (solve_box_qp_admm_torch.py:349-432)
// ---------------------------------------------------------------------------
template <typename T> struct BwdParams {
    int B, n, m, N, Np, K;
    const T *g, *x, *u, *lams, *nus, *Q, *A, *lb, *ub, *rho_in;
    T rho_value;
    int rho_mode;
    T *dQ, *dp, *dA, *db, *dlb, *dub;
    T* M;        // B * Np * Np
    T* packed;
    T* rhs;      // B * Np  (rhs, then the solution d)
    int *piv, *dest, *info;
    int* fidx;   // B * n : indices of the free variables (reduced system), in order
    int* nred;   // B     : size of the reduced system = #free + m
    int reduced; // 1: solve on the free set only
    int chol;    // 1: the reduced system is solved through a blocked Cholesky of Q_FF (f32, symmetric Q)
    T* rhs2;     // B * Np: residual / correction of the one refinement step of the LU form (or null)
    int refine;  // 1: the epilogue adds rhs2 to rhs
    unsigned long long* dbg;   // optional cycle counters (8 per problem), debug only
    int la_maxk;               // largest block count the look-ahead Cholesky may take (LDS of the launch), 0 = off
    T* bsc;                    // Cholesky form: [B][Np] the power-of-two equilibration of the free-set block, S (Q_FF + eps I) S (0 = off)
    int* host_report;          // optional pinned host memory, B ints: the epilogue leaves every problem's info word there
    int early_report;          // 1: Cholesky form -- k_bwd_chol_solve reports right behind its factorisation, not the epilogue
    int reported;              // 1 (phase 2 only): the phase-1 call has stored the info words into host_report already
    int lu_reported;           // 1: LU form -- k_report_info has stored them right behind the factorisation, the epilogue does not
    int phase;                 // Cholesky form in two calls: 1 = free set + Q_FF + its factorisation only (no cotangent needed:
                               // enqueued right behind the forward), 2 = the solves + epilogue on that factor; 0 = everything
    int kkt;                   // 1: the KKT-system backward (backward='kkt', reference :435-584) on the same kernels: the (3n+m)
                               //    system [[Q, G^T diag(lam), A^T], [G, -diag(s), 0], [A, 0, 0]] with G = [-I; I] reduces exactly
                               //    (dlam = diag(1/s) G dx) to [[Q + diag(w), A^T], [A, 0]] [dx; dnu] = [-g; 0],
                               //    w = lam_lo / s_lo + lam_hi / s_hi (both clamped at 1e-8, :450-452): every variable is "free",
                               //    w takes the place of the 1e-8 regulariser, and the epilogue forms dlb / dub from dlam
    int piv_cols;              // 1: the look-ahead Cholesky's last pivot block stops behind the last free variable (LQP_PIV_COLS)
    const T* curv;             // B * n or null (lqp_boxqp_backward_fp_curv): a non-negative diagonal h added to the 1e-8 of every FREE variable --
                               //    the system is [[Q_FF + diag(h_F), A_F^T], [A_F, 0]] (+1e-8 I), the Hessian of a smooth separable term of the
                               //    objective (the log barrier: w / x^2); the builds, the Cholesky form's equilibration and the refinement's
                               //    residual read it; null = the expressions as they were; never together with kkt
};

// diagonal weight of the KKT-system backward for variable i (see BwdParams::kkt)
template <typename T>
__device__ __forceinline__ T kkt_weight(const BwdParams<T>& P, const int b, const int i) {
    const int n = P.n;
    const T xi = P.x[(size_t)b * n + i];
    const T slo = tmax(xi - P.lb[(size_t)b * n + i], T(1e-8)), shi = tmax(P.ub[(size_t)b * n + i] - xi, T(1e-8));
    const T llo = tmax(P.lams[(size_t)b * 2 * n + i], T(1e-8)), lhi = tmax(P.lams[(size_t)b * 2 * n + n + i], T(1e-8));
    return llo / slo + lhi / shi;
}

template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_bwd_build(const BwdParams<T> P) {
    // mask :360-365, rhs :368-375, non-symmetric system :378-392
    const int b = blockIdx.x, n = P.n, m = P.m, Np = P.Np;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const T rho = (P.rho_mode == 2) ? P.rho_in[b] : P.rho_value;
    const T* x = P.x + (size_t)b * n;
    const T* u = P.u + (size_t)b * n;
    const T* lb = P.lb + (size_t)b * n;
    const T* ub = P.ub + (size_t)b * n;
    const T* g = P.g + (size_t)b * n;
    const T* Q = P.Q + (size_t)b * n * n;
    const T* A = P.A ? P.A + (size_t)b * m * n : nullptr;
    T* M = P.M + (size_t)b * Np * Np;
    T* rhs = P.rhs + (size_t)b * Np;
    const T* cv = P.curv ? P.curv + (size_t)b * n : nullptr;
    if (tid == 0) P.info[b] = 0;
    const bool qvec = (n % 4 == 0) && ((((uintptr_t)Q) % sizeof(V4<T>)) == 0);
#pragma unroll 2
    for (int i = w; i < n; i += LQP_NW) {
        const T s = x[i] + u[i];
        const T keep = (s > ub[i] || s < lb[i]) ? T(0) : T(1);
        const T* qr = Q + (size_t)i * n;
        T* mr = M + (size_t)i * Np;
        if (qvec) {
            for (int j = lane * 4; j < n; j += 256) {
                V4<T> v = *(const V4<T>*)(qr + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    T val = keep * v.v[e];
                    if (j + e == i) val = (val + rho * (T(1) - keep)) + (cv ? T(1e-8) + keep * cv[i] : T(1e-8));
                    v.v[e] = val;
                }
                *(V4<T>*)(mr + j) = v;
            }
        } else {
            for (int j = lane; j < n; j += 64) {
                T val = keep * qr[j];
                if (j == i) val = (val + rho * (T(1) - keep)) + (cv ? T(1e-8) + keep * cv[i] : T(1e-8));
                mr[j] = val;
            }
        }
        for (int r = lane; r < m; r += 64) mr[n + r] = keep * A[(size_t)r * n + i];
        if (lane == 0) rhs[i] = -(g[i] * keep);
    }
    for (int r = w; r < m; r += LQP_NW) {
        T* mr = M + (size_t)(n + r) * Np;
        for (int j = lane; j < n; j += 64) mr[j] = A[(size_t)r * n + j];
        for (int c = lane; c < m; c += 64) mr[n + c] = (c == r) ? T(1e-8) : T(0);
        if (lane == 0) rhs[n + r] = T(0);
    }
}

// Reduced fixed-point system.  For an active bound (keep_i = 0) row i of the reference's system
// (:378-392) reads (rho + 1e-8) dv_i = 0, so dv_i = 0 exactly and the variable drops out of every
// other row: what is left is [[Q_FF, A_F^T], [A_F, 0]] (+1e-8 I) [dv_F; dnu] = [-g_F; 0] on the
// free set F.  Same solution, (|F|+m)^3 instead of (n+m)^3 work.  LDS: fl[n] (int) | wtot[NW]
template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_bwd_build_reduced(const BwdParams<T> P) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, n = P.n, m = P.m, Np = P.Np;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int* fl = (int*)smem;               // free list
    int* wtot = fl + round_up(n, 8);
    const T* x = P.x + (size_t)b * n;
    const T* u = P.u + (size_t)b * n;
    const T* lb = P.lb + (size_t)b * n;
    const T* ub = P.ub + (size_t)b * n;
    const T* g = P.g + (size_t)b * n;
    const T* Q = P.Q + (size_t)b * n * n;
    const T* A = P.A ? P.A + (size_t)b * m * n : nullptr;
    T* M = P.M + (size_t)b * Np * Np;
    T* rhs = P.rhs + (size_t)b * Np;
    if (tid == 0 && blockIdx.y == 0) P.info[b] = 0;
    // ---- ordered compaction of the free set: one variable per thread and pass (n <= 1024: one pass) ----
    int nf = 0;
    for (int i0 = 0; i0 < n; i0 += LQP_NT) {
        const int i = i0 + tid;
        bool keep = false;
        if (i < n) {
            if (P.kkt) keep = true;
            else {
                const T sxu = x[i] + u[i];
                keep = !(sxu > ub[i] || sxu < lb[i]);
            }
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (i0 > 0) __syncthreads();                  // (wtot of the previous pass has been read by everybody)
        if (lane == 0) wtot[w] = __popcll(bal);
        __syncthreads();
        int base = nf;
#pragma unroll
        for (int ww = 0; ww < LQP_NW; ++ww) {
            const int c = wtot[ww];
            if (ww < w) base += c;
            nf += c;
        }
        if (keep) {
            fl[base + before] = i;
            if (blockIdx.y == 0) P.fidx[(size_t)b * n + base + before] = i;
        }
    }
    if (tid == 0 && blockIdx.y == 0) P.nred[b] = nf + m;
    __syncthreads();
    // ---- reduced matrix and right-hand side (rows interleaved over the gridDim.y workgroups) ----
    const int wy = blockIdx.y, ny = gridDim.y;
    // (two rows per wave at a time, eight gathers of each in flight before the first store -- clamped indices, no guarded load:
    //  one gather, its wait and its store per trip were ~5 memory round trips per row, 56 us at n = 500)
    constexpr int GQ = 8;
    for (int a0 = (w * ny + wy) * 2; a0 < nf; a0 += LQP_NW * ny * 2) {
        const int a1 = a0 + 1 < nf ? a0 + 1 : a0;
        const int i0 = fl[a0], i1 = fl[a1];
        const T* q0 = Q + (size_t)i0 * n;
        const T* q1 = Q + (size_t)i1 * n;
        const T dg0 = P.kkt ? kkt_weight(P, b, i0) : P.curv ? T(1e-8) + P.curv[(size_t)b * n + i0] : T(1e-8);
        const T dg1 = P.kkt ? kkt_weight(P, b, i1) : P.curv ? T(1e-8) + P.curv[(size_t)b * n + i1] : T(1e-8);
        for (int c0 = 0; c0 < nf; c0 += 64 * GQ) {
            T v0[GQ], v1[GQ];
#pragma unroll
            for (int q = 0; q < GQ; ++q) {
                const int c = c0 + lane + 64 * q;
                const int col = fl[c < nf ? c : nf - 1];
                v0[q] = q0[col];
                v1[q] = q1[col];
            }
#pragma unroll
            for (int q = 0; q < GQ; ++q) {
                const int c = c0 + lane + 64 * q;
                if (c < nf) {
                    M[(size_t)a0 * Np + c] = c == a0 ? v0[q] + dg0 : v0[q];
                    if (a1 != a0) M[(size_t)a1 * Np + c] = c == a1 ? v1[q] + dg1 : v1[q];
                }
            }
        }
        for (int r = lane; r < m; r += 64) {
            M[(size_t)a0 * Np + nf + r] = A[(size_t)r * n + i0];
            if (a1 != a0) M[(size_t)a1 * Np + nf + r] = A[(size_t)r * n + i1];
        }
        if (lane == 0 && P.g) { rhs[a0] = -g[i0]; if (a1 != a0) rhs[a1] = -g[i1]; }      // (no cotangent yet: phase 1, k_bwd_gather_rhs later)
    }
    for (int r = w * ny + wy; r < m; r += LQP_NW * ny) {
        T* mr = M + (size_t)(nf + r) * Np;
        for (int c = lane; c < nf; c += 64) mr[c] = A[(size_t)r * n + fl[c]];
        for (int c = lane; c < m; c += 64) mr[nf + c] = (c == r && !P.kkt) ? T(1e-8) : T(0);
        if (lane == 0) rhs[nf + r] = T(0);
    }
}

// ---------------------------------------------------------------------------
// Cholesky form of the reduced backward system (f32, Q symmetric, n <= 1024, m <= 16):
//   [[Kf, A_F^T], [A_F, eps I]] [dv_F; dnu] = [-g_F; 0],   Kf = Q_FF + eps I  (eps = 1e-8, :378-392)
//   dv_F = u0 - G dnu,  u0 = Kf^-1 (-g_F),  G = Kf^-1 A_F^T,  (A_F G - eps I) dnu = A_F u0.
// Build: ordered compaction of the free set, Kf as packed lower 64x64 blocks (identity padding), -g_F -> rhs,
// A_F rows -> the (otherwise unused) M buffer.  LDS: fl[n] (int) | wtot[NW]
// ---------------------------------------------------------------------------
// Symmetric equilibration of the backward's free-set block by POWERS OF TWO: s_a = 2^-floor(log2(d_a) / 2), d_a the diagonal entry
// (q_aa + 1e-8, or + the KKT form's weight), so that every diagonal entry of S (Q_FF + eps I) S lies in [1, 4).  Exact in floating
// point -- the float32 Cholesky factorisation sees the same significands, its roundoff is invariant -- and it is what lets the
// float16-pipe tile products scale a 32-row block by ONE factor: the reference's Q is not pre-conditioned in the backward
// (:378-393), and rows 10^3 apart in magnitude inside a block lost up to ten bits there (measured on D Q D, d = 10^U(-1.5, 1.5):
// dp 5e-5 of scale against 5e-7).  The system solved is S K S (S^-1 dv) = S rhs, the equality rows enter as A_F S.
__device__ __forceinline__ float bwd_equil_scale(const float d) {
    if (!(d > 0.f) || !(d < 3.0e38f)) return 1.f;
    const int h = (int)((__float_as_uint(d) >> 23) & 0xFFu) - 127;       // floor(log2 d)
    return __uint_as_float((unsigned int)(127 - (h >> 1)) << 23);
}
template <int LQP_ANY = 0>      // (a template only so that the split build can place its one instance: tools/gen_split_build.py)
__global__ __launch_bounds__(LQP_NT) void k_bwd_build_chol(const BwdParams<float> P) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, n = P.n, m = P.m, Np = P.Np;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int* fl = (int*)smem;
    int* wtot = fl + round_up(n, 8);
    const float* x = P.x + (size_t)b * n;
    const float* u = P.u + (size_t)b * n;
    const float* lb = P.lb + (size_t)b * n;
    const float* ub = P.ub + (size_t)b * n;
    const float* g = P.g + (size_t)b * n;
    const float* Q = P.Q + (size_t)b * n * n;
    const float* A = P.A ? P.A + (size_t)b * m * n : nullptr;
    const int Kmax = round_up(n, LQP_NB) / LQP_NB, Npm = Kmax * LQP_NB;
    float* Ls = P.packed + (size_t)b * sym_blocks(Kmax) * LQP_BLK;
    float* AF = P.M + (size_t)b * Np * Np;
    float* rhs = P.rhs + (size_t)b * Np;
    if (tid == 0 && blockIdx.y == 0) P.info[b] = 0;
    float* wl = (float*)(wtot + LQP_NW + 8);          // KKT-system backward / a caller's curvature: the diagonal weights (n floats)
    const bool dwt = P.kkt || P.curv;                 // (the diagonal comes from wl, not the constant)
    bool keep = false;
    if (tid < n) {
        if (P.kkt) { keep = true; wl[tid] = kkt_weight(P, b, tid); }
        else {
            const float sxu = x[tid] + u[tid];
            keep = !(sxu > ub[tid] || sxu < lb[tid]);
            if (P.curv) wl[tid] = 1e-8f + P.curv[(size_t)b * n + tid];
        }
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = __popcll(bal);
    __syncthreads();
    int base = 0, nf = 0;
#pragma unroll
    for (int ww = 0; ww < LQP_NW; ++ww) {
        const int c = wtot[ww];
        if (ww < w) base += c;
        nf += c;
    }
    if (keep) {
        fl[base + before] = tid;
        if (blockIdx.y == 0) P.fidx[(size_t)b * n + base + before] = tid;
    }
    if (tid == 0 && blockIdx.y == 0) P.nred[b] = nf + m;
    __syncthreads();
    const int Kb = round_up(nf, LQP_NB) / LQP_NB;
    const int r = tid >> 4, c4 = (tid & 15) * 4;
    const int nblk = sym_blocks(Kb);
    // the equilibration (bwd_equil_scale): s of free variable a, 1 on the padding; kept for the solve kernel
    float* const sl = wl + round_up(n, 8);
    for (int a = tid; a < Npm; a += LQP_NT) {
        float sv = 1.f;
        if (P.bsc && a < nf) sv = bwd_equil_scale(Q[(size_t)fl[a] * n + fl[a]] + (dwt ? wl[fl[a]] : 1e-8f));
        sl[a] = sv;
        if (P.bsc && blockIdx.y == 0) P.bsc[(size_t)b * Np + a] = sv;
    }
    __syncthreads();
    for (int t = blockIdx.y; t < nblk; t += gridDim.y) {
        int j = 0;
        while (sym_idx(j + 1, j + 1, Kb) <= t && j + 1 < Kb) ++j;      // block column of stream position t
        const int i = j + (t - sym_idx(j, j, Kb));
        const int a = i * 64 + r;
        // (unconditional gathers with clamped indices, then a select: a guarded load costs a branch and a full
        //  s_waitcnt per element)
        const bool rok = a < nf;
        const size_t rowoff = (size_t)fl[rok ? a : 0] * n;
        float q4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = j * 64 + c4 + e;
            q4[e] = Q[rowoff + fl[c < nf ? c : 0]];
        }
        V4<float> v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = j * 64 + c4 + e;
            float val = (a == c) ? 1.f : 0.f;
            if (rok && c < nf) val = ((q4[e] + (a == c ? (dwt ? wl[fl[a]] : 1e-8f) : 0.f)) * sl[a]) * sl[c];
            v.v[e] = val;
        }
        *(V4<float>*)(Ls + (size_t)t * LQP_BLK + tid * 4) = v;
    }
    if (blockIdx.y == 0) {
        if (P.phase != 1)          // (phase 1: no cotangent yet -- k_bwd_chol_solve gathers it in phase 2)
            for (int a = tid; a < Npm; a += LQP_NT) rhs[a] = a < nf ? -g[fl[a]] * sl[a] : 0.f;
        for (int q = 0; q < m; ++q)
            for (int a = tid; a < Npm; a += LQP_NT) AF[(size_t)q * Npm + a] = a < nf ? A[(size_t)q * n + fl[a]] * sl[a] : 0.f;
    }
}

// factor + solves + Schur complement of the equality rows; leaves [dv_F; dnu] in rhs like the LU path
// LDS: wg_chol_factor's layout, then v | acc | u0 | G[m][Npm] | t[64] | part[NW*64] | S[m*m] | wv[m] | dn[m]
// (nr: right-hand sides solved together, 2 or 4 -- see k_bwd_chol_solve)
__host__ __device__ inline int bwd_chol_lds_bytes(int n, int m, int nr = 2) {
    const int Kmax = round_up(n, LQP_NB) / LQP_NB, Npm = Kmax * LQP_NB;
    const int a0 = spd_lds_bytes(Kmax > SPD_MAXK ? SPD_MAXK : Kmax);      // (above: wg_chol_factor_big, panel in chunks)
    const int a = (Kmax < SPD_MAXK && chol_la_lds_bytes(Kmax) > a0) ? chol_la_lds_bytes(Kmax) : a0;
    const int c = ((1 + nr + m) * Npm + nr * 64 + nr * LQP_NW * 64 + m * m + 2 * m + 8) * 4;
    return a > c ? a : c;
}
// NRV = 0: the 1 + m solves two right-hand sides at a time (the headline's m = 1: one round); NRV = 4: four at a time, an instance
// of its own for problems with three or more equality rows (m = 16: five rounds of block-column barriers instead of nine) -- its
// registers are not the m <= 2 kernel's problem.  The same arithmetic per right-hand side either way.
// F16 (round 6): the look-ahead factorisation's tile waves on the float16 matrix pipe (wg_chol_factor_la<true>)
template <int NRV = 0, bool F16 = false>
__global__ __launch_bounds__(LQP_NT) void k_bwd_chol_solve(const BwdParams<float> P) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, n = P.n, m = P.m, Np = P.Np;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Kmax = round_up(n, LQP_NB) / LQP_NB, Npm = Kmax * LQP_NB;
    const int nf = P.nred[b] - m;
    const int Kb = round_up(nf, LQP_NB) / LQP_NB, Nb = Kb * LQP_NB;
    float* Ls = P.packed + (size_t)b * sym_blocks(Kmax) * LQP_BLK;
    const float* AF = P.M + (size_t)b * Np * Np;
    float* rhs = P.rhs + (size_t)b * Np;
    unsigned long long dt0 = P.dbg ? clock64() : 0;
    if (Kb > 0 && P.phase != 2) {
        if (Kb <= P.la_maxk) wg_chol_factor_la<F16>(Ls, Kb, P.info + b, smem, P.dbg ? P.dbg + (size_t)b * 8 : nullptr, P.piv_cols ? nf : 0);
        else if (Kb <= SPD_MAXK) wg_chol_factor(Ls, Kb, P.info + b, smem);
        else wg_chol_factor_big(Ls, Kb, P.info + b, smem);
    }
    // The factorisation is what can fail (Q_FF not positive definite in float32: the caller repeats on the pivoted LU): its info
    // word goes to the caller's pinned host memory NOW -- of the prefactor call when there was one (phase 1; phase 2 then finds
    // P.reported) --, so that a synchronous caller, which polls those words, returns while the solves and the epilogue still run
    // (stream-ordered results) and prepares its next call under them.  What the Schur complement of the equality rows can still
    // find below (a pivot that is not a positive number: with its -1e-8 I that is a NaN, i.e. NaN inputs) is not reported
    // any more: the epilogue poisons that problem's gradients with NaN, which is what the reference's solve hands back for it.
    if (P.host_report && (P.early_report || P.phase == 1) && !P.reported) {      // (a prefactor call always reports)
        __syncthreads();
        if (tid == 0)
            __hip_atomic_store(P.host_report + b, __hip_atomic_load(P.info + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (P.phase == 1) return;              // (the factor is in the workspace: lqp_boxqp_backward_fp_prefactor)
    __syncthreads();
    if (P.dbg && tid == 0) { const unsigned long long t = clock64(); P.dbg[(size_t)b * 8 + 0] = t - dt0; dt0 = t; P.dbg[(size_t)b * 8 + 3] = Kb; }
    // right-hand sides [rhs | A_F^T] as rows of X (u0 = X[0], G = X[1 ..]), solved two at a time
    constexpr int NR = NRV == 4 ? 4 : 2;
    float* acc = (float*)smem;
    float* u0 = acc + (size_t)NR * Npm;
    float* G = u0 + Npm;
    float* t = G + (size_t)m * Npm;
    float* part = t + NR * 64;
    float* S = part + NR * LQP_NW * 64;
    float* wv = S + m * m;
    float* dn = wv + m;
    auto fill = [&]() {                    // (wg_chol_solve_all: ahead of its request for the factor's blocks and a barrier; at most one element per thread and loop)
        if (P.phase == 2) {                // the cotangent arrives only now: gathered over the free set of phase 1
            const float* g = P.g + (size_t)b * n;
            const int* fidx = P.fidx + (size_t)b * n;
            const float* bs_ = P.bsc ? P.bsc + (size_t)b * Np : nullptr;
#pragma unroll 1
            for (int e = tid; e < Nb; e += LQP_NT) u0[e] = e < nf ? -g[fidx[e]] * (bs_ ? bs_[e] : 1.f) : 0.f;
        } else {
#pragma unroll 1
            for (int e = tid; e < Nb; e += LQP_NT) u0[e] = rhs[e];
        }
        for (int q = 0; q < m; ++q)
#pragma unroll 1
            for (int e = tid; e < Nb; e += LQP_NT) G[(size_t)q * Npm + e] = AF[(size_t)q * Npm + e];
    };
    wg_chol_solve_all<NR>(Ls, Kb, u0, Npm, 1 + m, acc, t, part, true, fill,
                          (P.dbg && P.la_maxk == 0) ? P.dbg + (size_t)b * 8 : nullptr);
    if (P.dbg && tid == 0) { const unsigned long long t = clock64(); P.dbg[(size_t)b * 8 + 1] = t - dt0; dt0 = t; }
    if (m > 0) {
        // S = A_F G - eps I,  wv = A_F u0  (one wave per entry)
        for (int e = w; e < m * m + m; e += LQP_NW) {
            const int q = e < m * m ? e / m : e - m * m;
            const float* rv = e < m * m ? G + (size_t)(e - q * m) * Npm : u0;
            float a = 0.f;
            for (int i = lane; i < nf; i += 64) a += AF[(size_t)q * Npm + i] * rv[i];
            a = wave_sum(a);
            if (lane == 0) {
                if (e < m * m) S[e] = a - ((e / m == e % m) ? 1e-8f : 0.f);
                else wv[q] = a;
            }
        }
        __syncthreads();
        // (S - eps I) dnu = wv: Gauss-Jordan with partial pivoting, m <= 16.  One thread per entry of [S | wv] (a single thread walked
        // through all of it before: ~4 m^3 dependent LDS round trips, 0.2 ms of the 0.3 ms kernel at m = 16); the same operations on
        // the same values per entry, so the same bits.  dn[0] doubles as the pivot row, dn[1] as the skip flag of a column step.
        {
            const int rr = tid / (m + 1), jj = tid - rr * (m + 1);          // entry (rr, jj); jj == m: the right-hand side
            const bool mine = tid < m * (m + 1);
            int* pivrow = (int*)dn;
            for (int c = 0; c < m; ++c) {
                if (tid == 0) {
                    int pr = c;
                    float best = tabs(S[c * m + c]);
                    for (int r2 = c + 1; r2 < m; ++r2) if (tabs(S[r2 * m + c]) > best) { best = tabs(S[r2 * m + c]); pr = r2; }
                    const bool skip = !(best > 0.f);
                    if (skip && P.info[b] == 0) P.info[b] = nf + c + 1;
                    pivrow[0] = pr; pivrow[1] = skip ? 1 : 0;
                }
                __syncthreads();
                const int pr = pivrow[0];
                const bool skip = pivrow[1] != 0;
                float* const rowc = jj < m ? S + c * m + jj : wv + c;        // this thread's column of rows c / pr / rr
                float* const rowp = jj < m ? S + pr * m + jj : wv + pr;
                float* const rowr = jj < m ? S + rr * m + jj : wv + rr;
                if (!skip && pr != c && tid <= m) {                          // swap rows c and pr (threads 0 .. m: rr == 0, one column each)
                    const float tmp = *rowc; *rowc = *rowp; *rowp = tmp;
                }
                __syncthreads();
                const float inv = skip ? 0.f : 1.f / S[c * m + c];
                const float f = (mine && !skip) ? S[rr * m + c] : 0.f;       // (read before anybody writes column c)
                __syncthreads();
                if (!skip && tid <= m) *rowc *= inv;
                __syncthreads();
                if (mine && !skip && rr != c) *rowr -= f * *rowc;
                __syncthreads();
            }
            for (int q = tid; q < m; q += LQP_NT) dn[q] = wv[q];
        }
        __syncthreads();
    }
    for (int a = tid; a < nf; a += LQP_NT) {
        float d = u0[a];
        for (int q = 0; q < m; ++q) d -= G[(size_t)q * Npm + a] * dn[q];
        rhs[a] = P.bsc ? d * P.bsc[(size_t)b * Np + a] : d;             // dv = S (the solution of the equilibrated system)
    }
    for (int q = tid; q < m; q += LQP_NT) rhs[nf + q] = dn[q];
    if (P.dbg && tid == 0) P.dbg[(size_t)b * 8 + 2] = clock64() - dt0;
}

// test aid (lqp_debug_chol_solve): the block solves of k_bwd_chol_solve alone, on the caller's packed factors and right-hand sides.
// reg = 0: wg_chol_solve_n whatever the block count.  LDS: acc[NR * Npm] | X[nrhs * Npm] | t[NR * 64] | part[NR * NW * 64]
__host__ __device__ inline int debug_chol_solve_lds_bytes(int Kmax, int nrhs, int nr) {
    return ((nr + nrhs) * Kmax * LQP_NB + nr * 64 + nr * LQP_NW * 64) * 4;
}
template <int NR>
__global__ __launch_bounds__(LQP_NT) void k_debug_chol_solve(const float* __restrict__ packed, const int* __restrict__ kb,
                                                             const float* __restrict__ V, float* __restrict__ Xo, const int Kmax,
                                                             const int nrhs, const int reg) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, Npm = Kmax * LQP_NB;
    const int K = min(max(kb[b], 0), Kmax), Nb = K * LQP_NB;
    const float* Ls = packed + (size_t)b * sym_blocks(Kmax) * LQP_BLK;
    const float* Vb = V + (size_t)b * nrhs * Npm;
    float* Xb = Xo + (size_t)b * nrhs * Npm;
    float* acc = (float*)smem;
    float* X = acc + (size_t)NR * Npm;
    float* t = X + (size_t)nrhs * Npm;
    float* part = t + NR * 64;
    auto fill = [&]() {
        for (int c = 0; c < nrhs; ++c)
            for (int e = tid; e < Nb; e += LQP_NT) X[(size_t)c * Npm + e] = Vb[(size_t)c * Npm + e];
    };
    wg_chol_solve_all<NR>(Ls, K, X, Npm, nrhs, acc, t, part, reg != 0, fill);
    for (int c = 0; c < nrhs; ++c)
        for (int e = tid; e < Npm; e += LQP_NT) Xb[(size_t)c * Npm + e] = e < Nb ? X[(size_t)c * Npm + e] : 0.f;
}

// test aid (lqp_debug_chol_factor): the factorisation k_bwd_chol_solve chooses for Kb = ceil(nf / 64) alone, in place on the caller's
// lower blocks (sym_idx(i, j, Kb) of each problem's sym_blocks(Kmax) blocks, the last block padded with the identity as
// k_bwd_build_chol pads it).  cols = 0: every pivot block takes its 64 columns; 1: the last one stops behind column nf.
template <bool F16>
__global__ __launch_bounds__(LQP_NT) void k_debug_chol_factor(float* __restrict__ packed, const int* __restrict__ nf,
                                                              int* __restrict__ info, const int Kmax, const int la_maxk, const int cols) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x;
    const int nfb = min(max(nf[b], 0), Kmax * LQP_NB);
    const int Kb = round_up(nfb, LQP_NB) / LQP_NB;
    float* Ls = packed + (size_t)b * sym_blocks(Kmax) * LQP_BLK;
    if (Kb == 0) return;
    if (Kb <= la_maxk) wg_chol_factor_la<F16>(Ls, Kb, info + b, smem, nullptr, cols ? nfb : 0);
    else wg_chol_factor(Ls, Kb, info + b, smem);
}

// One step of iterative refinement for the LU form of the reduced system: r = rhs - M d with the ORIGINAL entries
// (Q, A gathered again; M itself was factored in place), dot products accumulated in double.  The cached solve uses
// explicitly inverted 64x64 diagonal blocks, which -- like any fp32 LU of this bordered, nearly singular-cornered
// matrix -- leaves 1e-5 ... 1e-4 of error when the exact dv is ~0 (dl_dz in the row space of A); one correction
// solve with the same factor brings it to the fp32 rounding level.  LDS: dvf[n] | dn[m] | fl[n] (int)
template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_bwd_residual(const BwdParams<T> P) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, n = P.n, m = P.m, Np = P.Np;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    T* dvf = (T*)smem;                     // dv scattered to all n variables (0 on the active set)
    T* dn = dvf + round_up(n, 8);
    int* fl = (int*)(dn + round_up(m > 0 ? m : 1, 8));
    const int nf = P.nred[b] - m;
    const T* d = P.rhs + (size_t)b * Np;
    T* r = P.rhs2 + (size_t)b * Np;
    const T* Q = P.Q + (size_t)b * n * n;
    const T* A = P.A ? P.A + (size_t)b * m * n : nullptr;
    const T* g = P.g + (size_t)b * n;
    for (int i = tid; i < n; i += LQP_NT) dvf[i] = T(0);
    for (int a = tid; a < nf; a += LQP_NT) fl[a] = P.fidx[(size_t)b * n + a];
    for (int q = tid; q < m; q += LQP_NT) dn[q] = d[nf + q];
    __syncthreads();
    for (int a = tid; a < nf; a += LQP_NT) dvf[fl[a]] = d[a];
    __syncthreads();
    // gridDim.y == 2: two workgroups per problem, alternate groups of rows (at B <= 128 half the CUs are idle).  Four rows per
    // wave at a time, their loads issued together (a row at a time was one memory round trip + reduction per row: 31 in sequence
    // at n = 500); each row's terms are added in the order they always were.
    constexpr int RG = 4;
    const int ny = (int)gridDim.y, me = (int)blockIdx.y;
    for (int a0 = (w * ny + me) * RG; a0 < nf + m; a0 += LQP_NW * ny * RG) {
        const T* row[RG];
        double acc[RG];
#pragma unroll
        for (int u = 0; u < RG; ++u) {
            const int a = min(a0 + u, nf + m - 1);
            row[u] = a >= nf ? A + (size_t)(a - nf) * n : Q + (size_t)fl[a] * n;
            acc[u] = 0.0;
        }
        for (int j = lane; j < n; j += 64) {
            const double dj = (double)dvf[j];
            T v[RG];
#pragma unroll
            for (int u = 0; u < RG; ++u) v[u] = row[u][j];
#pragma unroll
            for (int u = 0; u < RG; ++u) acc[u] += (double)v[u] * dj;
        }
#pragma unroll
        for (int u = 0; u < RG; ++u) acc[u] = wave_sum(acc[u]);
        if (lane < RG && a0 + lane < nf + m) {
            const int a = a0 + lane;
            double mine = readlane_t(acc[0], 0);          // (lane 0's sums: the bits the one-row form produced)
#pragma unroll
            for (int u = 1; u < RG; ++u) { const double t = readlane_t(acc[u], 0); mine = lane == u ? t : mine; }
            double res;
            if (a < nf) {
                const int i = fl[a];
                res = -(double)g[i] - mine - (P.curv ? (double)(T(1e-8) + P.curv[(size_t)b * n + i]) : 1e-8) * (double)d[a];
                for (int q = 0; q < m; ++q) res -= (double)A[(size_t)q * n + i] * (double)dn[q];
            } else {
                res = -mine - 1e-8 * (double)dn[a - nf];
            }
            r[a] = (T)res;
        }
    }
    if (me == 0)
        for (int a = nf + m + tid; a < Np; a += LQP_NT) r[a] = T(0);
}

// solve with the packed factor (one rhs per problem, in global memory, in place)
// LDS: v[Np] | tmp[64] | dest[Np]
template <typename T> __host__ __device__ inline int solve_lds_bytes(int Np) { return (Np + 64) * (int)sizeof(T) + Np * 4; }

template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_packed_solve(const T* __restrict__ packed_all, const int Nuni, const int Npmax,
                                                         const int Kmax, const int* __restrict__ dest_all,
                                                         T* __restrict__ rhs_all, const int nrhs,
                                                         const size_t rhs_bstride, const int rhs_rstride,
                                                         const int rhs_cstride, const int* __restrict__ Nvec) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = Nvec ? Nvec[b] : Nuni;
    const int K = round_up(N, LQP_NB) / LQP_NB, Np = K * LQP_NB;
    T* v = (T*)smem;
    T* tmp = v + Npmax;
    int* dest = (int*)(tmp + 64);
    const T* packed = packed_all + (size_t)b * packed_blocks(Kmax) * LQP_BLK;
    const int S = K * (K + 1);
    const bool cyclic = true;                 // (wg_packed_solve pads the stream to a multiple of the ring depth)
    BlockStream<T, LQP_NT> st;
    stream_prime(st, packed, S);
    for (int i = tid; i < Np; i += LQP_NT) dest[i] = dest_all[(size_t)b * Npmax + i];
    __syncthreads();
    T* rhs = rhs_all + (size_t)b * rhs_bstride;
    for (int c = 0; c < nrhs; ++c) {
        for (int i = tid; i < Np; i += LQP_NT) v[dest[i]] = (i < N) ? rhs[(size_t)i * rhs_rstride + (size_t)c * rhs_cstride] : T(0);
        wg_barrier_lds();
        wg_packed_solve(st, packed, K, v, tmp, cyclic && (c + 1 < nrhs));
        if (!cyclic && c + 1 < nrhs) stream_prime(st, packed, S);
        for (int i = tid; i < N; i += LQP_NT) rhs[(size_t)i * rhs_rstride + (size_t)c * rhs_cstride] = v[i];
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_bwd_epilogue(const BwdParams<T> P) {
    // gradients :396-430; d = [dv; dnu] is in P.rhs
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int b = blockIdx.x, n = P.n, m = P.m, Np = P.Np;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    T* dv = (T*)smem;          // n
    T* xs = dv + n;            // n
    T* dnu = xs + n;           // m
    const T rho = (P.rho_mode == 2) ? P.rho_in[b] : P.rho_value;
    const T* d = P.rhs + (size_t)b * Np;
    const T* x = P.x + (size_t)b * n;
    // singular system / Q_FF not positive definite: gradients come out as NaN, never as plausible garbage
    const T poison = P.info[b] != 0 ? T(__builtin_nanf("")) : T(0);
    if (P.host_report && !(P.chol && P.early_report) && !P.lu_reported && tid == 0 && blockIdx.y == 0)      // (straight into pinned host memory: no device-to-host copy behind the
                                                                       //  call; Cholesky form: k_bwd_chol_solve has reported already)
        __hip_atomic_store(P.host_report + b, P.info[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (P.reduced) {
        const int nf = P.nred[b] - m;
        const int* fl = P.fidx + (size_t)b * n;
        const T* d2 = P.rhs2 + (size_t)b * Np;           // correction of the refinement step (LU form)
        for (int i = tid; i < n; i += LQP_NT) { dv[i] = poison; xs[i] = x[i]; }
        __syncthreads();
        for (int a = tid; a < nf; a += LQP_NT) dv[fl[a]] = d[a] + (P.refine ? d2[a] : T(0)) + poison;
        for (int r = tid; r < m; r += LQP_NT) dnu[r] = d[nf + r] + (P.refine ? d2[nf + r] : T(0)) + poison;
    } else {
        for (int i = tid; i < n; i += LQP_NT) { dv[i] = d[i] + poison; xs[i] = x[i]; }
        for (int r = tid; r < m; r += LQP_NT) dnu[r] = d[n + r] + poison;
    }
    __syncthreads();
    // gridDim.y workgroups share the rows of one problem (dQ is a pure 4 n^2-byte write); the small outputs: slab 0
    const bool first = blockIdx.y == 0;
    if (P.dp && first) for (int i = tid; i < n; i += LQP_NT) P.dp[(size_t)b * n + i] = dv[i];
    if (P.db && first) for (int r = tid; r < m; r += LQP_NT) P.db[(size_t)b * m + r] = -dnu[r];
    if (P.dA && m > 0 && first) {
        const T* nus = P.nus + (size_t)b * m;
        for (int t = tid; t < m * n; t += LQP_NT) {
            const int r = t / n, j = t - r * n;
            P.dA[(size_t)b * m * n + t] = dnu[r] * xs[j] + nus[r] * dv[j];
        }
    }
    const T* Q = P.Q + (size_t)b * n * n;
    const T* A = P.A ? P.A + (size_t)b * m * n : nullptr;
    if (P.kkt && first) {
        // dlam = diag(1 / s) G dx (rows -I | I), dl_dh = -lam dlam, dlb = -dl_dh[:n], dub = dl_dh[n:] (:544, :573-575)
        for (int i = tid; i < n; i += LQP_NT) {
            const T xi = xs[i];
            const T slo = tmax(xi - P.lb[(size_t)b * n + i], T(1e-8)), shi = tmax(P.ub[(size_t)b * n + i] - xi, T(1e-8));
            const T llo = tmax(P.lams[(size_t)b * 2 * n + i], T(1e-8)), lhi = tmax(P.lams[(size_t)b * 2 * n + n + i], T(1e-8));
            if (P.dlb) P.dlb[(size_t)b * n + i] = llo * (-dv[i] / slo);
            if (P.dub) P.dub[(size_t)b * n + i] = -lhi * (dv[i] / shi);
        }
    }
    const bool need_kkt = (P.dlb || P.dub) && !P.kkt;
    T* dQ = P.dQ ? P.dQ + (size_t)b * n * n : nullptr;
    // 16-B stores; a lane's columns are the same in every row, so their x_j and dv_j / 2 stay in registers
    const bool vec = (n % 4 == 0) && n <= 1024 && dQ && ((((uintptr_t)dQ) % sizeof(V4<T>)) == 0);
    V4<T> xj[4], hj[4];
    if (vec) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane * 4 + 256 * q;
#pragma unroll
            for (int e = 0; e < 4; ++e) { xj[q].v[e] = j < n ? xs[j + e] : T(0); hj[q].v[e] = j < n ? T(0.5) * dv[j + e] : T(0); }
        }
    }
    for (int i = w + LQP_NW * blockIdx.y; i < n; i += LQP_NW * gridDim.y) {
        const T hi = T(0.5) * dv[i], xi = xs[i];
        T acc = T(0);
        if (need_kkt) {
            const T* qr = Q + (size_t)i * n;
            for (int j = lane; j < n; j += 64) acc += qr[j] * dv[j];
            acc = wave_sum(acc);
        }
        if (dQ) {
            T* o = dQ + (size_t)i * n;
            if (vec) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = lane * 4 + 256 * q;
                    if (j < n) {
                        V4<T> ov;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ov.v[e] = hi * xj[q].v[e] + hj[q].v[e] * xi;
                        *(V4<T>*)(o + j) = ov;
                    }
                }
            } else {
                for (int j = lane; j < n; j += 64) o[j] = hi * xs[j] + (T(0.5) * dv[j]) * xi;
            }
        }
        if (need_kkt && lane == 0) {
            T kkt = -P.g[(size_t)b * n + i] - acc;
            T at = T(0);
            for (int r = 0; r < m; ++r) at += A[(size_t)r * n + i] * dnu[r];
            if (m > 0) kkt = kkt - at;
            T div = rho * P.u[(size_t)b * n + i];
            if (div == T(0)) div = T(1);
            const T dlam = kkt / div;
            const T* lams = P.lams + (size_t)b * 2 * n;
            if (P.dlb) P.dlb[(size_t)b * n + i] = dlam * lams[i];
            if (P.dub) P.dub[(size_t)b * n + i] = -dlam * lams[n + i];
        }
    }
}

// ---------------------------------------------------------------------------
// KKT solve helpers (lqp_py/solve_qp_eqcon_torch.py:23-25, utils.py:23-32)
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_kkt_build(const T* __restrict__ Qall, const T* __restrict__ pall,
                                                      const T* __restrict__ Aall, const T* __restrict__ ball,
                                                      const int n, const int m, const int Np,
                                                      T* __restrict__ Mall, T* __restrict__ rhsall, int* info) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const T* Q = Qall + (size_t)b * n * n;
    T* M = Mall + (size_t)b * Np * Np;
    T* rhs = rhsall + (size_t)b * Np;
    if (tid == 0) info[b] = 0;
    for (int i = w; i < n; i += LQP_NW) {
        const T* qr = Q + (size_t)i * n;
        T* mr = M + (size_t)i * Np;
        for (int j = lane; j < n; j += 64) mr[j] = qr[j];
        for (int r = lane; r < m; r += 64) mr[n + r] = Aall[(size_t)b * m * n + (size_t)r * n + i];
        if (lane == 0) rhs[i] = -pall[(size_t)b * n + i];
    }
    for (int r = w; r < m; r += LQP_NW) {
        T* mr = M + (size_t)(n + r) * Np;
        for (int j = lane; j < n; j += 64) mr[j] = Aall[(size_t)b * m * n + (size_t)r * n + j];
        for (int c = lane; c < m; c += 64) mr[n + c] = T(0);
        if (lane == 0) rhs[n + r] = ball[(size_t)b * m + r];
    }
}

template <typename T>
__global__ void k_kkt_unpack(const T* __restrict__ rhsall, const int n, const int m, const int Np,
                             T* __restrict__ x, T* __restrict__ nus) {
    const int b = blockIdx.x;
    const T* d = rhsall + (size_t)b * Np;
    for (int i = threadIdx.x; i < n; i += blockDim.x) x[(size_t)b * n + i] = d[i];
    if (nus) for (int r = threadIdx.x; r < m; r += blockDim.x) nus[(size_t)b * m + r] = d[n + r];
}

// dQ = 0.5 (dx x^T + x dx^T); dA = dnu x^T + nus dx^T
template <typename T>
__global__ __launch_bounds__(LQP_NT) void k_outer_grads(const T* __restrict__ dx, const T* __restrict__ x,
                                                        const T* __restrict__ dnu, const T* __restrict__ nus,
                                                        const int n, const int m, T* __restrict__ dQ, T* __restrict__ dA) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const T* dxb = dx + (size_t)b * n;
    const T* xb = x + (size_t)b * n;
    if (dQ) {
        for (int i = w; i < n; i += LQP_NW) {
            const T di = dxb[i], xi = xb[i];
            T* o = dQ + (size_t)b * n * n + (size_t)i * n;
            for (int j = lane; j < n; j += 64) o[j] = T(0.5) * (di * xb[j] + xi * dxb[j]);
        }
    }
    if (dA && m > 0) {
        for (int t = tid; t < m * n; t += LQP_NT) {
            const int r = t / n, j = t - r * n;
            dA[(size_t)b * m * n + t] = dnu[(size_t)b * m + r] * xb[j] + nus[(size_t)b * m + r] * dxb[j];
        }
    }
}

// strided copies between a user (B,N,N) matrix and the padded workspace
template <typename T>
__global__ void k_copy_matrix(const T* __restrict__ src, const int lds_, const size_t sstride,
                              T* __restrict__ dst, const int ldd, const size_t dstride, const int N) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = w; i < N; i += nw)
        for (int j = lane; j < N; j += 64) dst[(size_t)b * dstride + (size_t)i * ldd + j] = src[(size_t)b * sstride + (size_t)i * lds_ + j];
}
// phase 2 of the LU form: the right-hand side [-g_F; 0] over the free set phase 1 left in the workspace (what k_bwd_build_reduced
// writes itself when it has the cotangent)
template <typename T>
__global__ __launch_bounds__(256) void k_bwd_gather_rhs(const BwdParams<T> P) {
    const int b = blockIdx.x, n = P.n, m = P.m;
    const int nf = P.nred[b] - m;
    const T* g = P.g + (size_t)b * n;
    const int* fl = P.fidx + (size_t)b * n;
    T* rhs = P.rhs + (size_t)b * P.Np;
    for (int a = threadIdx.x; a < nf; a += 256) rhs[a] = -g[fl[a]];
    for (int r = threadIdx.x; r < m; r += 256) rhs[nf + r] = T(0);
}

// the info words of a factorisation into the caller's pinned host memory (LU form of the backward: they are final behind the LU, a
// synchronous caller that polls them returns while pack, solves and epilogue still run)
// ---------------------------------------------------------------------------
// backward of lqp_boxqp_forward_l1: two element-wise kernels around lqp_boxqp_backward_fp, which runs unchanged in between.
// An element on the kink (side == 0) behaves like one whose two bounds are both c; a thresholded free element like p shifted by
// side * w.  So: the effective box (lb_e, ub_e) = K ? (c, c) : (lb, ub) with the dual u_e = K ? u : u_box and its lams ...
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_l1_effective_box(const T* __restrict__ side, const T* __restrict__ u, const T* __restrict__ ubox,
                                                          const T* __restrict__ lb, const T* __restrict__ ub, const T* __restrict__ c,
                                                          const T* __restrict__ rho_in, const T rho_value, const int n, const size_t total,
                                                          T* __restrict__ lb_e, T* __restrict__ ub_e, T* __restrict__ u_e,
                                                          T* __restrict__ lams_e) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / n, e = i - b * n;
    const bool K = side[i] == T(0);
    const T ue = K ? u[i] : ubox[i];
    lb_e[i] = K ? c[i] : lb[i];
    ub_e[i] = K ? c[i] : ub[i];
    u_e[i] = ue;
    lams_from_y(lams_e, b, n, e, (rho_in ? rho_in[b] : rho_value) * ue);
}
// ... and what the effective box's gradients mean for the eight inputs: on K both bounds were c (dc = dlb_e + dub_e, nothing for
// lb and ub), elsewhere they were the bounds; dw = side * dp.  Outputs may be null; dlb / dub may be dlb_e / dub_e themselves.
template <typename T>
__global__ __launch_bounds__(256) void k_l1_finish_grads(const T* __restrict__ side, const T* __restrict__ dp, const T* dlb_e, const T* dub_e,
                                                         const size_t total, T* dlb, T* dub, T* __restrict__ dc, T* __restrict__ dw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const T s = side[i];
    const bool K = s == T(0);
    const T gl = dlb_e[i], gu = dub_e[i];
    if (dlb) dlb[i] = K ? T(0) : gl;
    if (dub) dub[i] = K ? T(0) : gu;
    if (dc) dc[i] = K ? gl + gu : T(0);
    if (dw) dw[i] = s * dp[i];
}

// backward of lqp_boxqp_forward_soft, the same recipe with two kink sets: Kl = (zone == -1) rests on lo, Kh = (zone == +1) on hi; both
// behave like an element whose two bounds are that kink.  A sloped free element (zone == +-2) is p shifted by wu / -wl.  A kink that
// lies beyond a hard bound holds nothing: the bound does (u_box != 0), and the element is an ordinary clamped one -- not in K.
template <typename T>
__global__ __launch_bounds__(256) void k_soft_effective_box(const T* __restrict__ zone, const T* __restrict__ u, const T* __restrict__ ubox,
                                                            const T* __restrict__ lb, const T* __restrict__ ub, const T* __restrict__ lo,
                                                            const T* __restrict__ hi, const T* __restrict__ rho_in, const T rho_value,
                                                            const int n, const size_t total, T* __restrict__ lb_e, T* __restrict__ ub_e,
                                                            T* __restrict__ u_e, T* __restrict__ lams_e) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / n, e = i - b * n;
    const T zn = zone[i];
    const bool held = ubox[i] != T(0);
    const bool Kl = zn == T(-1) && !held, Kh = zn == T(1) && !held, K = Kl || Kh;
    const T kv = Kh ? hi[i] : lo[i];
    const T ue = K ? u[i] : ubox[i];
    lb_e[i] = K ? kv : lb[i];
    ub_e[i] = K ? kv : ub[i];
    u_e[i] = ue;
    lams_from_y(lams_e, b, n, e, (rho_in ? rho_in[b] : rho_value) * ue);
}
// ... and the ten inputs' gradients from the effective box's: on a kink both bounds were the kink (its gradient dlb_e + dub_e, nothing
// for lb and ub); dwu = dp on zone == +2, dwl = -dp on zone == -2.  Outputs may be null; dlb / dub may be dlb_e / dub_e themselves.
template <typename T>
__global__ __launch_bounds__(256) void k_soft_finish_grads(const T* __restrict__ zone, const T* __restrict__ ubox, const T* __restrict__ dp, const T* dlb_e, const T* dub_e,
                                                           const size_t total, T* dlb, T* dub, T* __restrict__ dwl, T* __restrict__ dwu,
                                                           T* __restrict__ dlo, T* __restrict__ dhi) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const T zn = zone[i];
    const bool held = ubox[i] != T(0);
    const bool Kl = zn == T(-1) && !held, Kh = zn == T(1) && !held, K = Kl || Kh;
    const T gl = dlb_e[i], gu = dub_e[i], g = dp[i];
    if (dlb) dlb[i] = K ? T(0) : gl;
    if (dub) dub[i] = K ? T(0) : gu;
    if (dlo) dlo[i] = Kl ? gl + gu : T(0);
    if (dhi) dhi[i] = Kh ? gl + gu : T(0);
    if (dwu) dwu[i] = zn == T(2) ? g : T(0);
    if (dwl) dwl[i] = zn == T(-2) ? -g : T(0);
}

// backward of lqp_boxqp_forward_pwl, the same recipe with a kink set per kink: K_k = (piece == 2 k - 1) rests on kink k (`c`: [K][B][n], the
// caller's K <= PWL_K kinks; a padded kink holds nothing: its jump is zero); a free element on a slope (piece == 2 k) is p shifted
// by s_k.  As for the band, an element a hard bound holds (u_box != 0) is an ordinary clamped one, whatever kink lies there.
template <typename T>
__global__ __launch_bounds__(256) void k_pwl_effective_box(const T* __restrict__ piece, const T* __restrict__ u, const T* __restrict__ ubox,
                                                           const T* __restrict__ lb, const T* __restrict__ ub, const T* __restrict__ c, const int K,
                                                           const T* __restrict__ rho_in, const T rho_value, const int n, const size_t total,
                                                           T* __restrict__ lb_e, T* __restrict__ ub_e, T* __restrict__ u_e,
                                                           T* __restrict__ lams_e) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / n, e = i - b * n;
    const int pc = (int)piece[i];
    const bool on = (pc & 1) && pc >= 1 && pc < 2 * K && ubox[i] == T(0);      // (bounded: `piece` is data)
    const T kv = on ? c[(size_t)(pc >> 1) * total + i] : T(0);
    const T ue = on ? u[i] : ubox[i];
    lb_e[i] = on ? kv : lb[i];
    ub_e[i] = on ? kv : ub[i];
    u_e[i] = ue;
    lams_from_y(lams_e, b, n, e, (rho_in ? rho_in[b] : rho_value) * ue);
}
// ... and the eight inputs' gradients from the effective box's: on kink k both bounds were c_k (dc_k = dlb_e + dub_e, nothing for lb
// and ub); ds_k = dp where piece == 2 k.  ds: [K + 1][B][n], dc: [K][B][n], every slot written.  Outputs may be null; dlb / dub
// may be dlb_e / dub_e themselves.
template <typename T>
__global__ __launch_bounds__(256) void k_pwl_finish_grads(const T* __restrict__ piece, const T* __restrict__ ubox, const T* __restrict__ dp, const T* dlb_e,
                                                          const T* dub_e, const int K, const size_t total, T* dlb, T* dub, T* __restrict__ ds, T* __restrict__ dc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pc = (int)piece[i];
    const bool on = (pc & 1) && ubox[i] == T(0);
    const T gl = dlb_e[i], gu = dub_e[i], g = dp[i];
    if (dlb) dlb[i] = on ? T(0) : gl;
    if (dub) dub[i] = on ? T(0) : gu;
    if (ds) for (int k = 0; k <= K; ++k) ds[(size_t)k * total + i] = pc == 2 * k ? g : T(0);
    if (dc) for (int k = 1; k <= K; ++k) dc[(size_t)(k - 1) * total + i] = (on && pc == 2 * k - 1) ? gl + gu : T(0);
}

// backward of lqp_boxqp_forward_log: the fixed-point backward runs on the box's share of the dual (u_e = u_box: the clamped set is
// where it is not zero, whatever the barrier adds to u) with curv on the diagonal of the free-set block (lqp_boxqp_backward_fp_curv);
// lams_e is built from u_e as the forward builds lams
template <typename T>
__global__ __launch_bounds__(256) void k_log_effective_duals(const T* __restrict__ ubox, const T* __restrict__ rho_in, const T rho_value,
                                                             const int n, const size_t total, T* __restrict__ u_e, T* __restrict__ lams_e) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / n, e = i - b * n;
    const T ue = ubox[i];
    u_e[i] = ue;
    lams_from_y(lams_e, b, n, e, (rho_in ? rho_in[b] : rho_value) * ue);
}
// ... and dw from dp: the term's gradient is -w_i / x_i, so dw_i = -dp_i / z_i where w_i > 0, else 0 (at w_i = 0 the one-sided
// derivative is not defined when x_i <= 0: the convention of the header)
template <typename T>
__global__ __launch_bounds__(256) void k_log_finish_grads(const T* __restrict__ dp, const T* __restrict__ z, const T* __restrict__ w,
                                                          const size_t total, T* __restrict__ dw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (dw) dw[i] = w[i] > T(0) ? -dp[i] / z[i] : T(0);
}

// backward of lqp_boxqp_forward_huber: the log barrier's recipe (u_e = u_box, lams_e from it, the true box) with the term's own
// curvature, which is data of the zones: curv = w on the free elements of the quadratic zone (zone == 0, w > 0, u_box == 0), 0 on the
// linear pieces -- a constant force, p shifted by +-w delta -- and on a clamped element
template <typename T>
__global__ __launch_bounds__(256) void k_huber_effective_duals(const T* __restrict__ ubox, const T* __restrict__ zone, const T* __restrict__ w,
                                                               const T* __restrict__ rho_in, const T rho_value, const int n, const size_t total,
                                                               T* __restrict__ u_e, T* __restrict__ lams_e, T* __restrict__ curv) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / n, e = i - b * n;
    const T ue = ubox[i], wi = w[i];
    u_e[i] = ue;
    curv[i] = (zone[i] == T(0) && wi > T(0) && ue == T(0)) ? wi : T(0);
    lams_from_y(lams_e, b, n, e, (rho_in ? rho_in[b] : rho_value) * ue);
}
// ... and the term's three gradients from dp: the term's force on x is g = w clip(z - c, -delta, delta), so dw = dp clip(z - c, -delta,
// delta), dc = -w dp on the quadratic zone (0 on the linear pieces: g does not see c there) and ddelta = w zone dp.  Outputs may be null.
template <typename T>
__global__ __launch_bounds__(256) void k_huber_finish_grads(const T* __restrict__ dp, const T* __restrict__ z, const T* __restrict__ zone,
                                                            const T* __restrict__ w, const T* __restrict__ c, const T* __restrict__ delta,
                                                            const size_t total, T* __restrict__ dw, T* __restrict__ dc, T* __restrict__ ddelta) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const T g = dp[i], zn = zone[i], wi = w[i], dl = delta[i];
    if (dw) dw[i] = g * tmin(tmax(z[i] - c[i], -dl), dl);
    if (dc) dc[i] = zn == T(0) ? -wi * g : T(0);
    if (ddelta) ddelta[i] = wi * zn * g;
}

template <int LQP_ANY = 0>
__global__ void k_report_info(const int* __restrict__ info, int* __restrict__ host_report, const int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) __hip_atomic_store(host_report + i, info[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <typename TI>
__global__ void k_copy_ints(const TI* __restrict__ src, const int sstride, TI* __restrict__ dst, const int dstride, const int N) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < N; i += blockDim.x) dst[(size_t)b * dstride + i] = src[(size_t)b * sstride + i];
}

}  // namespace lqp
