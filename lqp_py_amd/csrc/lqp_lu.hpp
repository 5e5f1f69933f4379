// Batched LU with partial pivoting: one workgroup factors one N x N matrix in
// place (row-major, leading dimension ld, ld % 64 == 0), LAPACK getrf layout
// and 1-based pivots.  Replaces torch.linalg.lu_factor at
// lqp_py/solve_box_qp_admm_torch.py:215,254 and lqp_py/lu_layer.py:10,31.
//
// Right-looking, panel width PB:
//   1. panel  : thread t keeps the rows k0 + t + q * STRIDE, q < R, of the
//               panel in registers (R = 1 up to N = 1024: k_lu_factor; 2 and
//               4 above: k_lu_factor_big; 8 and 16 on four waves: the
//               several-workgroup kernels of lqp_lu_wide.hpp); per column a
//               wave max-|.| search (DPP inside 16-lane rows; first index
//               wins ties, as isamax), the pivot row is broadcast through
//               LDS, rank-1 update in registers (lu_panel_columns);
//   2. swaps  : the PB row interchanges are composed into one gather map
//               (lu_panel_store) and applied to the columns left and right
//               of the panel, a thread per column (lu_interchange_column);
//   3. U12    : the same threads solve L11 * U12 = (P A)12 in registers;
//   4. update : A22 -= L21 * U12 with L21^T and U12 staged in LDS: MFMA
//               32x32x2 f32 tiles (C tile prefetched one tile ahead and used
//               as the accumulator: D = C - L21 U12), or 8x4 VALU tiles.
#pragma once
#include "lqp_common.hpp"

namespace lqp {

template <typename T, int PB> struct LuLds {
    // byte offsets inside the dynamic LDS block, all multiples of 32
    int lt, up, l11, rowp, rowj, wval, wrcp, widx, wtid, pidx, src, xdst, xsrc, cnt, total;
    __host__ __device__ explicit LuLds(int Mpad) {
        int o = 0;
        lt = o;   o += PB * Mpad * (int)sizeof(T);
        up = o;   o += PB * Mpad * (int)sizeof(T);
        l11 = o;  o += round_up(PB * (PB + 1) * (int)sizeof(T), 32);
        rowp = o; o += 2 * LQP_NW * PB * (int)sizeof(T);       // candidate pivot rows [parity][wave][PB]
        rowj = o; o += round_up(2 * PB * (int)sizeof(T), 32);  // (not used; the slot keeps the layout the host sizes)
        wval = o; o += round_up(2 * LQP_NW * (int)sizeof(T), 32);
        wrcp = o; o += round_up(2 * LQP_NW * (int)sizeof(T), 32);
        widx = o; o += round_up(2 * LQP_NW * 4, 32);
        wtid = o; o += round_up(2 * LQP_NW * 4, 32);
        pidx = o; o += round_up(PB * 4, 32);
        src = o;  o += Mpad * 4;
        xdst = o; o += round_up(PB * 4, 32);
        xsrc = o; o += round_up(PB * 4, 32);
        cnt = o;  o += 32;
        total = o;
    }
};

// ---- wave-level arg-max without control flow --------------------------------
__device__ __forceinline__ float readlane_t(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ double readlane_t(double v, int l) {
    long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ float hwmax(float a, float b) { return fmaxf(a, b); }     // v_max_f32 (DPP-fusable)
__device__ __forceinline__ double hwmax(double a, double b) { return fmax(a, b); }
template <typename T> __device__ __forceinline__ T row16_max(T m) {
    m = hwmax(m, dpp<0xB1>(m));
    m = hwmax(m, dpp<0x4E>(m));
    m = hwmax(m, dpp<0x124>(m));
    m = hwmax(m, dpp<0x128>(m));
    return m;
}
__device__ __forceinline__ int row16_min_i32(int m) {
    m = min(m, dpp_i32<0xB1>(m));
    m = min(m, dpp_i32<0x4E>(m));
    m = min(m, dpp_i32<0x124>(m));
    m = min(m, dpp_i32<0x128>(m));
    return m;
}
// max of `key` over the wave (wave-uniform) and the LOWEST lane that holds it: with keys
// ordered by row this is isamax's "first index wins ties".
template <typename T> __device__ __forceinline__ void wave_argmax(const T key, T& best, int& lane_of_best) {
    const T m = row16_max(key);
    best = hwmax(hwmax(readlane_t(m, 0), readlane_t(m, 16)), hwmax(readlane_t(m, 32), readlane_t(m, 48)));
    lane_of_best = __ffsll((unsigned long long)__ballot(key == best)) - 1;
}

// MFMA trailing update (f32 only): each wave owns 32x32 tiles of A22.
// A operand (32x2 slice of L21): lane l holds L21[i = l&31][k = l>>5];
// B operand (2x32 slice of U12): lane l holds U12[k = l>>5][j = l&31];
// C/D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int PB, int NT>
__device__ __forceinline__ void lu_trailing_mfma_f32(float* __restrict__ A22, const int ld, const int M2,
                                                      const float* __restrict__ LT, const float* __restrict__ UP,
                                                      const int Mpad) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int nt = (M2 + 31) >> 5;
    const int ntiles = nt * nt;
    // lane part of every address (same for all 16 accumulator registers); the tile / register
    // part is wave-uniform and stays in SGPRs
    const int voff = 4 * lh * ld + li;
    auto load_c = [&](int t, f32x16& c) {
        const int ti = t / nt, tj = t - ti * nt;
        const float* base = A22 + (size_t)(ti << 5) * ld + (tj << 5);
        const bool colok = (tj << 5) + li < M2;
        const int rlim = M2 - (ti << 5) - 4 * lh;          // valid iff qrow < rlim
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int qrow = (q & 3) + 8 * (q >> 2);
            c[q] = (colok && qrow < rlim) ? base[(size_t)qrow * ld + voff] : 0.f;
        }
    };
    for (int t = __builtin_amdgcn_readfirstlane(w); t < ntiles; t += NT / 64) {
        f32x16 cur;
        load_c(t, cur);                         // in flight underneath the MFMA chain below
        const int ti = t / nt, tj = t - ti * nt;
        const int i0 = ti << 5, j0 = tj << 5;
        const float* lt = LT + i0 + li + lh * Mpad;
        const float* up = UP + j0 + li + lh * Mpad;
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
        for (int kk = 0; kk < PB; kk += 2) {
            const float a = lt[kk * Mpad];
            const float b = up[kk * Mpad];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        cur -= acc;
        float* base = A22 + (size_t)i0 * ld + j0;
        const bool colok = j0 + li < M2;
        const int rlim = M2 - i0 - 4 * lh;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int qrow = (q & 3) + 8 * (q >> 2);
            if (colok && qrow < rlim) base[(size_t)qrow * ld + voff] = cur[q];
        }
    }
}

// The same for float64: 16 x 16 tiles of v_mfma_f64_16x16x4_f64 (the one-workgroup kernels above 512 rows -- the sizes the
// two-workgroup LU does not take -- ran their trailing update on the vector unit: 4.0 ms per factorisation at N = 522, B = 128).
//   A operand (16x4 slice of L21): lane l holds L21[i = l & 15][k = l >> 4];  B operand: U12[k = l >> 4][j = l & 15];
//   C/D: lane l holds rows 4 q + (l >> 4), q = 0..3, of column l & 15 (tools/microbench/mfma_f64_layout.hip)
typedef double f64x4_lu __attribute__((ext_vector_type(4)));
template <int PB, int NT>
__device__ __forceinline__ void lu_trailing_mfma_f64(double* __restrict__ A22, const int ld, const int M2,
                                                      const double* __restrict__ LT, const double* __restrict__ UP,
                                                      const int Mpad) {
    static_assert(PB % 4 == 0, "panel width in steps of the instruction's depth");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 15, lh = lane >> 4;
    const int nt = (M2 + 15) >> 4;
    const int ntiles = nt * nt;
    for (int t = __builtin_amdgcn_readfirstlane(w); t < ntiles; t += NT / 64) {
        const int ti = t / nt, tj = t - ti * nt;
        const int i0 = ti << 4, j0 = tj << 4;
        double* base = A22 + (size_t)(i0 + lh) * ld + j0 + li;
        const bool colok = j0 + li < M2;
        const int rlim = M2 - i0 - lh;                    // register q holds row 4 q + lh
        f64x4_lu cur;
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = (colok && 4 * q < rlim) ? base[(size_t)(4 * q) * ld] : 0.0;
        const double* lt = LT + i0 + li + lh * Mpad;
        const double* up = UP + j0 + li + lh * Mpad;
        f64x4_lu acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < PB; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(lt[kk * Mpad], up[kk * Mpad], acc, 0, 0, 0);
        cur -= acc;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (colok && 4 * q < rlim) base[(size_t)(4 * q) * ld] = cur[q];
    }
}

// LDS scratch of the panel factorisation
template <typename T> struct PanelLds {
    T* rowP; T* wval; T* wrcp; int* widx; int* wtid; int* pidx; int* cnt;
};

// ---- the panel's rows, R per thread: row q of thread t is relative row t + q * STRIDE -------------------------------------
// `live`: this thread holds panel rows at all (the kernels whose panel runs on some of their waves only pass tid < STRIDE).
// A full panel (pb == PB) moves in 16-byte pieces: element by element every lane asked for its line PB times.
template <typename T, int PB, int R, int STRIDE>
__device__ __forceinline__ void lu_panel_load(V4<T> (&row4)[R][PB / 4], int (&curpos)[R], bool (&done)[R],
                                              const T* A, const int ld, const int k0, const int pb,
                                              const int M, const bool live) {
    typedef V4<T> vec;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        curpos[q] = (int)threadIdx.x + q * STRIDE;      // LAPACK position of this row
        done[q] = !(live && curpos[q] < M);             // already a pivot row (or no row at all)
    }
    if (pb == PB) {
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const T* rp = A + (size_t)(k0 + (int)threadIdx.x + q * STRIDE) * ld + k0;
#pragma unroll
            for (int v = 0; v < PB / 4; ++v) {
                if (!done[q]) row4[q][v] = *(const vec*)(rp + 4 * v);
                else { row4[q][v].v[0] = row4[q][v].v[1] = row4[q][v].v[2] = row4[q][v].v[3] = T(0); }
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const T* rp = A + (size_t)(k0 + (int)threadIdx.x + q * STRIDE) * ld + k0;
#pragma unroll
            for (int c = 0; c < PB; ++c) row4[q][c >> 2].v[c & 3] = (!done[q] && c < pb) ? rp[c] : T(0);
        }
    }
}

// The PB columns of one panel: unblocked factorisation, one column at a time.
// Rows never move between threads: a thread keeps the rows it loaded, `curpos` is the position LAPACK's explicit
// interchanges would have moved a row to, `done` marks rows already used as pivots.  Per column: the thread's best live
// row, wave arg-max of |a_rj| (ties: smallest position, as isamax), each wave's winner publishes its row, ONE barrier
// of the whole workgroup, cross-wave arg-max, branch-free rank-1 update against the broadcast pivot row.  Factoring goes
// on past a zero pivot (l = 0, as getf2); the first one is noted in cnt[1].  The publish buffers alternate with the
// column parity, so column j+1 never overwrites what a slow wave still reads for column j.
template <typename T, int PB, int R, int STRIDE>
__device__ __forceinline__ void lu_panel_columns(V4<T> (&row4)[R][PB / 4], int (&curpos)[R], bool (&done)[R],
                                                 const bool wact, const int pb, const int k0, const PanelLds<T>& S) {
    typedef V4<T> vec;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    T* const rowP = S.rowP; T* const wval = S.wval; T* const wrcp = S.wrcp;
    int* const widx = S.widx; int* const wtid = S.wtid; int* const pidx = S.pidx; int* const cnt = S.cnt;
#pragma unroll
    for (int j = 0; j < PB; ++j) {
        if (j < pb) {
            const int par = j & 1;
            T* cand = rowP + par * (LQP_NW * PB);
            T* wv = wval + par * LQP_NW;
            int* wi = widx + par * LQP_NW;
            int* wt = wtid + par * LQP_NW;
            T* wr = wrcp + par * LQP_NW;
            if (wact) {
                // this thread's best live row: largest |a_rj|, ties to the smaller position
                T aj = row4[0][j >> 2].v[j & 3];
                T key = done[0] ? T(-1) : tabs(aj);
                int cp = curpos[0], qs = 0;
#pragma unroll
                for (int q = 1; q < R; ++q) {
                    const T a = row4[q][j >> 2].v[j & 3];
                    const T kq = done[q] ? T(-1) : tabs(a);
                    const bool better = kq > key || (kq == key && kq >= T(0) && curpos[q] < cp);
                    if (better) { key = kq; aj = a; cp = curpos[q]; qs = q; }
                }
                T myrcp = T(1) / aj;                 // independent of the arg-max chain below
                asm volatile("" : "+v"(myrcp));      // keep it out of the winner-only branch
                T bw; int lb;
                wave_argmax(key, bw, lb);
                const unsigned long long tied = __ballot(key == bw);
                if (__popcll(tied) > 1) {                            // rare: smallest position wins
                    int c2 = (key == bw) ? cp : 0x7fffffff;
                    c2 = row16_min_i32(c2);
                    c2 = min(min(__builtin_amdgcn_readlane(c2, 0), __builtin_amdgcn_readlane(c2, 16)),
                             min(__builtin_amdgcn_readlane(c2, 32), __builtin_amdgcn_readlane(c2, 48)));
                    lb = __ffsll((unsigned long long)__ballot(key == bw && cp == c2)) - 1;
                }
                if (lane == lb) {
                    wv[w] = bw;
                    wr[w] = myrcp;
                    wi[w] = cp;
                    wt[w] = tid + qs * STRIDE;
#pragma unroll
                    for (int q4 = 0; q4 < PB / 4; ++q4) {
                        vec o = row4[0][q4];
#pragma unroll
                        for (int q = 1; q < R; ++q)
                            if (qs == q) o = row4[q][q4];
                        *(vec*)(cand + w * PB + 4 * q4) = o;
                    }
                }
            } else if (lane == 0) {
                wv[w] = T(-2);                                       // can never win
            }
            __syncthreads();
            if (wact) {
                // cross-wave arg-max: lane l looks at wave (l & 15)'s winner
                const T cv = wv[lane & 15];
                const int ci = wi[lane & 15];
                const int ct = wt[lane & 15];
                const T best = row16_max(cv);
                const unsigned long long tied = __ballot(cv == best) & 0xFFFFull;
                int ww = __ffsll(tied) - 1;
                if (__popcll(tied) > 1) {
                    const int c2 = row16_min_i32((cv == best) ? ci : 0x7fffffff);
                    ww = __ffsll((unsigned long long)__ballot(cv == best && ci == c2) & 0xFFFFull) - 1;
                }
                const int pivpos = __builtin_amdgcn_readlane(ci, ww);    // pivot row's position before the swap
                const int bi = __builtin_amdgcn_readlane(ct, ww);        // (thread + q * STRIDE) that owns the pivot row
                // the whole pivot row, 16 B per LDS read, all reads independent
                const T* rowPc = cand + ww * PB;
                vec pr[PB / 4];
#pragma unroll
                for (int q4 = j >> 2; q4 < PB / 4; ++q4) pr[q4] = *(const vec*)(rowPc + 4 * q4);
                const T rinv = wr[ww];
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    if (tid + q * STRIDE == bi) {
                        pidx[j] = pivpos;      // pivots / info go to global memory once per panel
                        if (!(best > T(0)) && cnt[1] == 0) cnt[1] = k0 + j + 1;
                        curpos[q] = j;
                        done[q] = true;
                    } else if (curpos[q] == j) {
                        curpos[q] = pivpos;    // the row that sat on the diagonal takes the pivot's old place
                    }
                    // branch-free elimination: finished rows (and a zero pivot column, as getf2) use l = 0
                    const bool upd = !done[q] && (best > T(0));
                    const T a = row4[q][j >> 2].v[j & 3];
                    const T l = upd ? a * rinv : T(0);
                    row4[q][j >> 2].v[j & 3] = upd ? l : a;
#pragma unroll
                    for (int c = j + 1; c < PB; ++c)
                        row4[q][c >> 2].v[c & 3] -= l * pr[c >> 2].v[c & 3];
                }
            }
        }
    }
}

// Write the factored panel back at its final position; stage L11 and L21^T in LDS; note the gather map of the
// interchanges: src (position -> original relative row) and the displaced top rows that ended below the panel top
// (xsrc -> xdst, *cnt of them; their sources are always < pb).
template <typename T, int PB, int R, int STRIDE>
__device__ __forceinline__ void lu_panel_store(const V4<T> (&row4)[R][PB / 4], const int (&curpos)[R],
                                               T* A, const int ld, const int k0, const int pb, const int M,
                                               const bool live, T* L11, T* LT, const int Mpad,
                                               int* src, int* xdst, int* xsrc,
                                               int* cnt) {
    typedef V4<T> vec;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int r = (int)threadIdx.x + q * STRIDE;
        if (live && r < M) {
            const int cp = curpos[q];
            T* wp = A + (size_t)(k0 + cp) * ld + k0;
            if (pb == PB) {
#pragma unroll
                for (int v = 0; v < PB / 4; ++v) *(vec*)(wp + 4 * v) = row4[q][v];
            } else {
#pragma unroll
                for (int c = 0; c < PB; ++c)
                    if (c < pb) wp[c] = row4[q][c >> 2].v[c & 3];
            }
            if (cp < pb) {
#pragma unroll
                for (int c = 0; c < PB; ++c) L11[cp * (PB + 1) + c] = row4[q][c >> 2].v[c & 3];
            } else {
#pragma unroll
                for (int c = 0; c < PB; ++c) LT[c * Mpad + (cp - pb)] = row4[q][c >> 2].v[c & 3];
            }
            src[cp] = r;
            if (cp >= pb && cp != r) {
                const int e = atomicAdd(cnt, 1);
                xdst[e] = cp;
                xsrc[e] = r;
            }
        }
    }
}

// does the panel move any row at all?  (wave-uniform)
template <int PB> __device__ __forceinline__ bool lu_any_interchange(const int* src, const int pb, const int ne) {
    bool any = ne > 0;
#pragma unroll
    for (int j = 0; j < PB; ++j)
        if (j < pb && __builtin_amdgcn_readfirstlane(src[j]) != j) any = true;
    return any;
}

// One column left (`right` false) or right of the panel, Ac = its element in row k0: apply the panel's interchanges and, right
// of the panel, solve L11 * U12 = (P A)12 for the column.  `top` holds the column's new top rows; `stage()` is the caller's store
// of them into its own U12 layout for the trailing update.  It runs BEFORE the rows go back to global memory: the barrier in
// front of the trailing update waits for the LDS stores only, and behind a queue of float64 global stores they arrived late.
template <typename T, int PB, typename STAGE>
__device__ __forceinline__ void lu_interchange_column(T* Ac, const int ld, const bool right, const int pb,
                                                      const int ne, const int* src,
                                                      const int* xsrc, const int* xdst,
                                                      const T* L11, T (&top)[PB], STAGE&& stage) {
    // (1) new top rows: sources anywhere in the panel rows
#pragma unroll
    for (int j = 0; j < PB; ++j)
        top[j] = (j < pb) ? Ac[(size_t)__builtin_amdgcn_readfirstlane(src[j]) * ld] : T(0);
    // (2) displaced top rows go down, at most 8 at a time (their sources are original top rows, which are only
    //     overwritten in step (4); ne <= pb, so panels of up to 8 columns take one trip)
    constexpr int G = PB < 8 ? PB : 8;
    for (int q0 = 0; q0 < ne; q0 += G) {
        T ext[G];
#pragma unroll
        for (int q = 0; q < G; ++q)
            ext[q] = (q0 + q < ne) ? Ac[(size_t)__builtin_amdgcn_readfirstlane(xsrc[q0 + q]) * ld] : T(0);
#pragma unroll
        for (int q = 0; q < G; ++q)
            if (q0 + q < ne) Ac[(size_t)__builtin_amdgcn_readfirstlane(xdst[q0 + q]) * ld] = ext[q];
    }
    // (3) U12 column: forward substitution with the unit-lower L11
    if (right) {
#pragma unroll
        for (int j = 0; j < PB; ++j) {
#pragma unroll
            for (int i = j + 1; i < PB; ++i) top[i] -= L11[i * (PB + 1) + j] * top[j];
        }
        stage();
    }
    // (4) store the new top rows
#pragma unroll
    for (int j = 0; j < PB; ++j)
        if (j < pb && (right || __builtin_amdgcn_readfirstlane(src[j]) != j)) Ac[(size_t)j * ld] = top[j];
}

// Trailing update on the vector unit: 8 x 4 tiles of A22 per thread.
template <typename T, int PB, int NT>
__device__ __forceinline__ void lu_trailing_valu(T* __restrict__ A22, const int ld, const int M2,
                                                 const T* __restrict__ LT, const T* __restrict__ UP, const int Mpad) {
    typedef V4<T> vec;
    const int tj_n = (M2 + 3) >> 2, ti_n = (M2 + 7) >> 3;
    for (int t = threadIdx.x; t < ti_n * tj_n; t += NT) {
        const int ti = t / tj_n, tj = t - ti * tj_n;
        const int i0 = ti << 3, j0 = tj << 2;
        T acc[8][4];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = T(0);
#pragma unroll 4
        for (int k = 0; k < PB; ++k) {
            const vec a0 = *(const vec*)(LT + k * Mpad + i0);
            const vec a1 = *(const vec*)(LT + k * Mpad + i0 + 4);
            const vec b0 = *(const vec*)(UP + k * Mpad + j0);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    acc[a][b] += a0.v[a] * b0.v[b];
                    acc[a + 4][b] += a1.v[a] * b0.v[b];
                }
        }
        const bool fullj = j0 + 3 < M2;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            if (i0 + a < M2) {
                T* p = A22 + (size_t)(i0 + a) * ld + j0;
                if (fullj) {
                    vec c = *(const vec*)p;
#pragma unroll
                    for (int b = 0; b < 4; ++b) c.v[b] -= acc[a][b];
                    *(vec*)p = c;
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + b < M2) p[b] -= acc[a][b];
                }
            }
        }
    }
}

// One workgroup of NT threads (512 or 1024) factors one matrix, R panel rows per thread: rows per panel N - k0 <= R * NT.
// R = 1 is the tuned kernel of N <= 1024; R = 2 takes 1024 < N <= 2048 and R = 4 float32 to 4096 (k_lu_factor_big: the
// matrix stays in global memory, 16 MB at N = 2048, and panels are lu_big_panel() or 4 columns wide so that L21^T and U12
// still fit in LDS).
// dbg (optional): 4 cycle counters per workgroup: panel, swaps+U12, trailing update, total
template <typename T, int PB, bool USE_MFMA, int NT, int R = 1>
__device__ __forceinline__ void wg_lu_factor(T* __restrict__ A, const int N, const int ld, int* __restrict__ ipiv,
                                             int* __restrict__ info, char* __restrict__ smem,
                                             unsigned long long* __restrict__ dbg) {
    // (N may come out of a per-problem size table, and then the LDS layout and every c * Mpad of the staging stores sit in vector
    //  registers across the whole factorisation.  A 1024-thread workgroup has 128 of them per thread and none to spare: float64
    //  with 16-column panels spills more than its ceiling in tests/test_abi_and_host.py without this.  512 threads have 256.)
    const int Mpad = NT == 1024 ? __builtin_amdgcn_readfirstlane(round_up(N, 64)) : round_up(N, 64);
    const LuLds<T, PB> L(Mpad);
    T* LT = (T*)(smem + L.lt);
    T* UP = (T*)(smem + L.up);
    T* L11 = (T*)(smem + L.l11);
    T* wval = (T*)(smem + L.wval);
    int* pidx = (int*)(smem + L.pidx);
    int* src = (int*)(smem + L.src);
    int* xdst = (int*)(smem + L.xdst);
    int* xsrc = (int*)(smem + L.xsrc);
    int* cnt = (int*)(smem + L.cnt);
    const PanelLds<T> S{(T*)(smem + L.rowp), wval, (T*)(smem + L.wrcp), (int*)(smem + L.widx), (int*)(smem + L.wtid), pidx, cnt};

    const int tid = threadIdx.x;
    const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);     // first row handled by this wave
    if (tid == 0) cnt[1] = 0;       // first zero pivot (1-based) seen by this factorisation, 0 = none
    if (tid < 2 * LQP_NW) wval[tid] = T(-2);     // slots of waves that do not exist (NT < 1024) never win
    unsigned long long t_panel = 0, t_swap = 0, t_trail = 0, t0 = 0, t_begin = 0;
    if (dbg) t_begin = clock64();

    for (int k0 = 0; k0 < N; k0 += PB) {
        const int pb = (N - k0 < PB) ? (N - k0) : PB;
        const int M = N - k0;
        const int M2 = M - pb;
        if (dbg) t0 = clock64();
        {
            // this thread's panel rows as PB/4 four-wide vectors: element c of row q = row4[q][c >> 2].v[c & 3]
            V4<T> row4[R][PB / 4];
            int curpos[R];
            bool done[R];
            const bool wact = wbase < M;   // this wave holds rows of the panel (wave-uniform)
            lu_panel_load<T, PB, R, NT>(row4, curpos, done, A, ld, k0, pb, M, true);
            if (tid == 0) *cnt = 0;
            lu_panel_columns<T, PB, R, NT>(row4, curpos, done, wact, pb, k0, S);
            lu_panel_store<T, PB, R, NT>(row4, curpos, A, ld, k0, pb, M, true, L11, LT, Mpad, src, xdst, xsrc, cnt);
        }
        __syncthreads();
        if (tid < pb) ipiv[k0 + tid] = k0 + pidx[tid] + 1;
        if (dbg) { const unsigned long long t1 = clock64(); t_panel += t1 - t0; t0 = t1; }
        const int ne = __builtin_amdgcn_readfirstlane(*cnt);
        const bool anyswap = lu_any_interchange<PB>(src, pb, ne);

        // ---- apply the interchanges left and right of the panel; U12 = L11^-1 (PA)12: one column at a time per thread ----
        for (int cc = tid; cc < N - pb; cc += NT) {
            const bool right = cc >= k0;
            const int col = right ? cc + pb : cc;
            if (right || anyswap) {
                T top[PB];
                lu_interchange_column<T, PB>(A + (size_t)k0 * ld + col, ld, right, pb, ne, src, xsrc, xdst, L11, top, [&] {
#pragma unroll
                    for (int j = 0; j < PB; ++j) UP[j * Mpad + (col - k0 - pb)] = top[j];
                });
            }
            // (N - pb <= NT at R = 1, one trip: said to the compiler, since a loop counter and its bound kept live across the
            //  column step put float64 with 16-column panels on 1024 threads over its spill ceiling in tests/test_abi_and_host.py)
            if constexpr (R == 1) break;
        }
        __syncthreads();
        if (dbg) { const unsigned long long t1 = clock64(); t_swap += t1 - t0; t0 = t1; }

        // ---- trailing update A22 -= L21 * U12 ----
        if (M2 > 0) {
            T* A22 = A + (size_t)(k0 + pb) * ld + (k0 + pb);
            if constexpr (USE_MFMA && sizeof(T) == 4) {
                lu_trailing_mfma_f32<PB, NT>((float*)A22, ld, M2, (const float*)LT, (const float*)UP, Mpad);
            } else if constexpr (USE_MFMA) {
                lu_trailing_mfma_f64<PB, NT>((double*)A22, ld, M2, (const double*)LT, (const double*)UP, Mpad);
            } else {
                lu_trailing_valu<T, PB, NT>(A22, ld, M2, LT, UP, Mpad);
            }
        }
        __syncthreads();
        if (dbg) { const unsigned long long t1 = clock64(); t_trail += t1 - t0; }
    }
    if (tid == 0 && cnt[1] != 0) *info = cnt[1];
    if (dbg && tid == 0) {
        dbg[0] = t_panel; dbg[1] = t_swap; dbg[2] = t_trail; dbg[3] = clock64() - t_begin;
    }
}

// panel width of the R > 1 forms (and of the several-workgroup kernels of lqp_lu_wide.hpp): 2 * PB * Mpad elements of LDS
template <typename T> __host__ __device__ constexpr int lu_big_panel() { return sizeof(T) == 4 ? 8 : 4; }

// (A look-ahead variant inside ONE workgroup -- waves 0-7 factoring panel k+1 while waves 8-15 ran panel k's trailing update -- was
//  measured no faster in rounds 1-2 and is gone from the sources; the look-ahead that pays runs on two CUs: lqp_lu2.hpp.)
// Panel width: L21^T and U12 (2 * PB * Mpad elements) must fit in LDS, and the panel row plus the
// broadcast pivot row (2 * PB elements per thread) must fit the register budget without spilling:
// 128 VGPRs in a 1024-thread workgroup (f32: 16 columns, f64: 8), 256 VGPRs in a 512-thread one
// (f32: 32, f64: 16).  Measured: a wider panel that spills loses to the narrower one.
template <typename T> __host__ __device__ inline int lu_threads(int N) { return N <= 512 ? 512 : 1024; }
template <typename T> __host__ __device__ inline int lu_panel_width(int N) {
    const int Mpad = round_up(N, 64);
    const int budget = 128 * 1024;
    const int widest = (sizeof(T) == 4 ? 16 : 8) * (lu_threads<T>(N) == 512 ? 2 : 1);
    if (widest >= 32 && 2 * 32 * Mpad * (int)sizeof(T) <= budget) return 32;
    if (widest >= 16 && 2 * 16 * Mpad * (int)sizeof(T) <= budget) return 16;
    return 8;
}

}  // namespace lqp
