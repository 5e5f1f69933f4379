// The ADMM loop of the symmetric path for n <= 128: k_admm_loop_small, an instance per form (FormAll ... FormL1)
#pragma once
#include "lqp_boxqp.hpp"

namespace lqp {

// ---------------------------------------------------------------------------
// The hot loop for SMALL problems (symmetric path, n <= 128: BASELINE configs[1], n = 100): the 1024-thread kernel above
// spends 8.4 k cycles per iteration there -- a 16-wave static walk with per-block LDS slots and partial-sum slices, sized
// for 36 blocks, around THREE blocks of work.  Here: 256 threads, the whole (unpacked, full) matrix -H in registers --
// thread t holds the 64 entries of row t >> 1, columns 64 (t & 1) .. -- the product is 64 FMAs per thread against
// broadcast reads of w and ONE lane-pair add; element e of every vector lives in thread e's registers (threads 0..127).
// Same iteration, same check (:285-313, blocking device-wide stop) and same exit state as admm_loop_body; first (hot)
// launch only, continuation launches (adaptive-rho events, a counter ring turn) run the general kernel.
// LDS: w[128] | y[128] | nus[m] | red[4 * 8 + 8]
// ---------------------------------------------------------------------------
__host__ __device__ inline int small_loop_lds_bytes(int m) { return (128 + 128 + (m > 0 ? m : 1) + 4 * 8 + 8 + 8) * 4; }
// FORM (FormAll ... FormLog), read as EACH, DETECT, DUAL and TERM below:
// EACH (control['stop'] = 'each'): the problem's own verdict ends its workgroup; no arrival word, no grid_wait
// DETECT (control['infeasible']): the certificate at every check, an instance of its own -- the loop has ONE body for hot and
// check iterations, and the certificate's registers in it cost the plain EACH kernel 12 % of its time
// DUAL (control['unbounded']): the dual certificate too
// FORM::term (lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber): the element-wise step with the separable term; keeps its thresholds beside lb / ub
template <typename FORM>
__device__ __forceinline__ void admm_loop_small_body(const FwdParams<float> P, const int it0, const int it1, const int ctr_base,
                                                     char* smem) {
    static constexpr bool EACH = FORM::each, DETECT = FORM::detect, DUAL = FORM::dual;      // (static: never a lambda's capture)
    using TERM = typename FORM::term;
    typedef float T;
    constexpr int NT = 256;
    const int b = blockIdx.x, n = P.n, m = P.m, Ks = P.Ks;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (__hip_atomic_load(P.status + ST_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    if constexpr (EACH) {          // this problem stopped in an earlier launch
        if (__builtin_amdgcn_readfirstlane(P.pstat[(size_t)b * PS_WORDS + PS_DONE])) return;
    }
    if (it0 >= it1) return;
    bool each_done = false;
    int each_why = 1;                   // (DETECT) 2 / 3: the problem stopped because it was flagged primal / dual infeasible
    int final_it = it1 - 1;
    T* const wv = (T*)smem;
    T* const yv = wv + 128;
    T* const nus_l = yv + 128;
    T* const red = nus_l + (m > 0 ? m : 1);
    VecView<T> V(P.vecs + (size_t)b * P.vstride, n, m);
    T* scal = P.scal + (size_t)b * SC_WORDS;
    const T* packed = P.packed + (size_t)b * packed_blocks(P.K) * LQP_BLK;
    const T rho = scal[SC_RHO];
    const T pnorm = scal[SC_PNORM];

    // ---- the full matrix: row r, columns 64 h .. 64 h + 63 (block (i, j) of the packed lower triangle, or the transpose
    //      of block (j, i)) ----
    const int r = tid >> 1, h = tid & 1;
    const int bi = r >> 6, rr = r & 63;
    const bool row_live = bi < Ks && h < Ks;
    T hreg[64];
    if (row_live) {
        if (bi >= h) {
            const T* src = packed + (size_t)sym_idx(bi, h, Ks) * LQP_BLK + rr * 64;
#pragma unroll
            for (int c = 0; c < 64; c += 4) {
                const V4<T> q = *(const V4<T>*)(src + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) hreg[c + e] = q.v[e];
            }
        } else {
            const T* src = packed + (size_t)sym_idx(h, bi, Ks) * LQP_BLK + rr;
#pragma unroll
            for (int c = 0; c < 64; ++c) hreg[c] = src[c * 64];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 64; ++c) hreg[c] = T(0);
    }
    // ---- element e = tid of every vector (threads 0..127) ----
    const int e = tid;
    const bool live = e < n;
    T zi = live ? V.z[e] : T(0), ui = live ? V.u[e] : T(0);
    const T psi = live ? V.ps[e] : T(0), lbi = live ? V.lbs[e] : T(0), ubi = live ? V.ubs[e] : T(0);
    const T di = live ? V.D[e] : T(1), cvi = (live && m > 0) ? V.cv[e] : T(0);
    typename TERM::template Regs<T> tr;           // (the term's thresholds; rho is this launch's: an adaptive-rho event ends it)
    if constexpr (TERM::kind != 0) { if (live) tr.load(P.termv + (size_t)b * term_stride<TERM>(n), n, e, rho); }
    T xi = T(0);
    if (tid < 128) { wv[tid] = live ? -psi + rho * (zi - ui) : T(0); }
    __syncthreads();

    int slot = ctr_base;
    for (int it = it0; it < it1; ++it) {
        const bool check = (it % P.check_solved) == 0;
        // ---- x-update: y = (-H) w, x = c - y ----
        {
            const T* wp = wv + 64 * h;
            T a0 = T(0), a1 = T(0);
#pragma unroll
            for (int c = 0; c < 64; c += 8) {
                const V4<T> q0 = *(const V4<T>*)(wp + c), q1 = *(const V4<T>*)(wp + c + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) { a0 += hreg[c + k] * q0.v[k]; a1 += hreg[c + 4 + k] * q1.v[k]; }
            }
            T acc = a0 + a1;
            acc += dpp<0xB1>(acc);                               // the two halves of a row sit in adjacent lanes
            if (h == 0 && r < 128) yv[r] = acc;
        }
        if ((check || it + 1 == it1) && m > 0) {                 // nu = T^T w - s0 (one wave per row) while wv still holds w
            for (int q = w; q < m; q += NT / 64) {
                T acc = T(0);
                for (int i = lane; i < n; i += 64) acc += V.Tm[(size_t)q * n + i] * wv[i];
                acc = wave_sum(acc);
                if (lane == 0) nus_l[q] = acc - V.s0[q];
            }
        }
        __syncthreads();
        T mx[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) mx[q] = T(0);
        T ia[4] = {T(0), T(0), T(0), T(0)};                      // (DETECT: the certificate's terms, see infeas_view)
        T da[4] = {T(0), T(0), T(0), T(0)};                      // (... and the dual certificate's, see dinf_elem)
        InfeasView<T> isv = {nullptr, nullptr, n, false, 0};
        if constexpr (DETECT) { if (check) isv = infeas_view(P, b, it, rho); }
        if (live) {
            const T wi = wv[e];
            xi = cvi - yv[e];
            const AdmmStep<T> sp = admm_step_term_tag<RelaxDyn, TERM>(P, xi, zi, ui, lbi, ubi, rho, tr);
            zi = sp.zn;
            ui = sp.un;
            if (check) {
                T qx = wi - rho * xi;
                for (int q = 0; q < m; ++q) qx -= V.As[(size_t)q * n + e] * nus_l[q];
                admm_step_norms<false>(mx, sp, xi, di, rho, qx);
                if constexpr (DETECT) { infeas_elem(ia, isv, e, rho * sp.un, qx + sp.s, lbi, ubi); if constexpr (DUAL) dinf_elem(da, isv, e, xi, qx, psi, lbi, ubi); }
            }
        }
        __syncthreads();                                         // (everybody has read w and y)
        if (tid < 128) wv[tid] = live ? -psi + rho * (zi - ui) : T(0);     // next right-hand side
        if (check) {
            T mv[6] = {mx[0], mx[1], mx[2], mx[3], mx[4], mx[5]};
            wg_max_n<T, 6, NT / 64>(mv, red);
            const LoopCheck<T> ck = loop_check(P, mv, pnorm);
            unsigned int* ct = P.counters + (size_t)slot * CT_WORDS;
            if constexpr (EACH) {
                if (tid == 0) {
                    loop_check_store<true>(P, scal, ck, mv, it);
                    if (!ck.solved) atomicAdd(ct + CT_NOTOPT, 1u);      // (k_check_done at the end of a host-driven chunk reads the slot)
                }
                ++slot;
                if constexpr (DETECT) {
                    const int flagged = infeas_finish<T, NT>(P, isv, ia, da, DUAL, nus_l, V.bs, it, rho, red);
                    if (flagged && !ck.solved) { each_done = true; each_why = flagged; final_it = it; break; }
                }
                if (ck.solved) { each_done = true; final_it = it; break; }      // (uniform: every thread holds the reduced norms)
            } else {
                ++slot;
                if (tid == 0) {
                    loop_check_store<false>(P, scal, ck, mv, it);
                    // the arrival and the verdict in ONE 64-bit add (NOTOPT and ARRIVE share an aligned word) behind the RETURNED adds:
                    // whoever sees the last arrival sees every counter of the check (see admm_loop_body)
                    unsigned int r1 = 0, r2 = 0;
                    if (ck.wants) r1 = atomicAdd(ct + CT_WANTS, 1u);
                    if (ck.trig) r2 = atomicAdd(ct + CT_TRIG, 1u);
                    asm volatile("s_waitcnt vmcnt(0)" :: "v"(r1), "v"(r2) : "memory");
                    __hip_atomic_fetch_add((unsigned long long*)(ct + CT_NOTOPT), (ck.solved ? 0ull : 1ull) | (1ull << 32),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (loop_all_optimal(P, ct, gridDim.x, it, b == 0 && tid == 0)) break;
            }
        }
        __syncthreads();
    }
    // ---- state for the continuation launch / the epilogue ----
    if (live) { V.z[e] = zi; V.u[e] = ui; V.x[e] = xi; }
    __syncthreads();
    for (int q = tid; q < m; q += NT) V.nu[q] = nus_l[q];
    if constexpr (EACH) {
        if (tid == 0) {
            if (each_done) each_stop(P, b, final_it, each_why);
            else P.pstat[(size_t)b * PS_WORDS + PS_FINAL] = final_it;      // (not optimal so far: the last iteration it ran)
        }
    }
}
template <typename FORM>
__global__ __launch_bounds__(256) void k_admm_loop_small(const FwdParams<float> P, const int it0, const int it1, const int ctr_base) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    admm_loop_small_body<FORM>(P, it0, it1, ctr_base, smem);
}

}  // namespace lqp
