// The ADMM loop of the symmetric path on two or four workgroups per problem, the matrix in their registers: k_admm_loop_split, an
// instance per form it has (FormAll, FormEach, FormL1, FormSoft, FormLog)
#pragma once
#include "lqp_boxqp.hpp"

namespace lqp {

// ---------------------------------------------------------------------------
// The same loop with TWO workgroups per QP (symmetric x-update, f32, 2 B <= #CUs, Ks >= SPLIT_MINK): workgroups b
// and b + B hold one half of the blocks of H each, ALL of them on chip for the whole launch (lqp_spd.hpp,
// wg_sym_gemv_split), and exchange their partial products every iteration:
//   thread e < Nps combines its element of this workgroup's partial, publishes it as ONE 8-byte granule
//   {tag, value} (agent-scope relaxed atomic store = sc1 write-through store), polls the partner's granule of the
//   same element (sc1 loads, L1 bypassed) until the tag matches, and adds the two partials in the fixed order
//   part 0 + part 1 -- both workgroups then hold bit-identical iterates and run the element-wise update and the
//   checks redundantly (part 0 alone reports to the counters / writes state).
// Two granule buffers alternate by iteration parity: a workgroup can be at most one exchange ahead of its
// partner, so a granule is never overwritten before it was read.  The area is zeroed by k_fwd_setup of the same
// forward (tags start at 1).  Spins are bounded: a timeout sets ST_TIMEOUT and the kernel still drains.
//
// The global stop (torch.all(is_optimal), :312) does not block the loop.  At a check, part 0 adds {not optimal?,
// arrival} to the check's counter word with ONE 64-bit atomic, both workgroups keep a snapshot of the iterate and go
// on iterating; in the following iterations part 0 reads the counter word while its product runs (the load's latency
// is hidden), and once all B arrivals are in, the verdict travels to the partner in the top bits of that iteration's
// granule tags.  "All optimal" -> both restore the snapshot, part 0 stores it and the kernel exits with the
// reference's iteration count (the 1-3 speculative iterations are dropped); otherwise the snapshot is forgotten.
// A verdict still open at the next check or at the last iteration of the launch is waited for (bounded spin).
//
// LDS (floats; every offset but the last three arrays is a compile-time constant):
//   [rl blocks] v yrow cvl part[NW][Nps] z u ps lb ub D xs sz su sx (Nps each) red[NW*8+8] flags[8] | bs nus snu (m each)
// ---------------------------------------------------------------------------
template <int NT, int NP = 2> __host__ __device__ constexpr int split_loop_lds_floats(int Ks) {
    return split_lds_blocks<NT, NP>(Ks) * LQP_BLK + (3 + NT / 64 + 10) * Ks * LQP_NB + (NT / 64) * 8 + 8 + 8;
}
template <int NT, int NP = 2> __host__ __device__ inline int split_loop_lds_bytes(int Ks, int m) {
    // + the equality block: As, G, T (m x Nps each), S, S^-1 (m x m), s0, b, nu, nu snapshot
    return (split_loop_lds_floats<NT, NP>(Ks) + 3 * m * Ks * LQP_NB + 2 * m * m + 4 * m + 8) * 4;
}
// NP = 4 (batches up to a quarter of the CUs): one column pair per workgroup, every partial product published once and
// fetched by the three others; the sum runs over the parts in their order on every workgroup (identical iterates).
// EACH (control['stop'] = 'each'): the partners hold bit-identical iterates and compute the same six norms, so each of them reaches the
// problem's verdict in the same iteration with no message: no arrival word, no snapshot, no look-back, no verdict in the tags (all
// compiled out).  Optimal -> the lead workgroup stores the iterate and marks pstat[b], every workgroup of the problem returns.  The hot
// launch ends at the first possible rho event (no hot_past): the continuation kernel (k_admm_loop, FormEach ...) takes the problem's own decision.
// (P by value: a reference to the kernel's parameter block costs the default's instances registers)
// FORM: FormAll, FormEach (which takes the certificates from P.snap and P.eps_dinf at run time: it serves FormDetect and FormCertify
// solves too) or a form with a separable term, FormL1 / FormSoft / FormLog / FormPwl / FormHuber (lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber: the element-wise step
// of every iteration form below with the term's prox; thread i keeps the term's Regs of its element, two / four / one / seven / four registers -- rho
// is this launch's, an event that changes it ends the launch)
template <int KS, int NT, bool DBG, int NP, typename FORM>
__device__ __forceinline__ void admm_loop_split_body(const FwdParams<float> P, int it0, const int it1, int ctr_base, char* smem) {
    typedef float T;
    static_assert(!FORM::detect, "the split loop's per-problem form reads the certificates at run time: FormEach is its instance");
    static constexpr bool EACH = FORM::each;      // (static: never a lambda's capture -- a generic lambda would take a plain local by reference)
    using TERM = typename FORM::term;
    if (P.hot_resume) {            // (a later round of the hot loop: it goes on where the round before stopped)
        const int r = __builtin_amdgcn_readfirstlane(P.status[ST_RESUME]);
        if (r <= 0) return;
        it0 = r;
        ctr_base = ((r + P.check_solved - 1) / P.check_solved) % P.ring;
    }
    constexpr int NWV = NT / 64, Ks = KS, Nps = KS * LQP_NB, rl = split_lds_blocks<NT, NP>(KS);
    constexpr int XPART = SPD_MAXK * LQP_NB, XPAR = NP * XPART;      // granules of one part / of one parity of the exchange
    // (split_seg: NP == 2)
    int b = 8 * ((int)blockIdx.x >> 4) + ((int)blockIdx.x & 7), part_id = ((int)blockIdx.x >> 3) & 1;      // (split_seg: shared_map with NP = 2)
    if (P.split_seg ? b >= P.B : !shared_map((int)blockIdx.x, P.B, NP, b, part_id)) return;
    const int n = P.n, m = P.m;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (__hip_atomic_load(P.status + ST_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    if constexpr (EACH) {          // this problem stopped in an earlier launch: every workgroup of it leaves
        if (__builtin_amdgcn_readfirstlane(P.pstat[(size_t)b * PS_WORDS + PS_DONE])) return;
    }
    if (!EACH && P.split_seg && P.seg_prev_slot >= 0) {
        // every problem was optimal at the last check (a launch enqueued ahead of that knowledge): as admm_loop_body
        if (__hip_atomic_load(P.counters + (size_t)P.seg_prev_slot * CT_WORDS + CT_NOTOPT, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) == 0) {
            if (blockIdx.x == 0 && tid == 0) {
                P.status[ST_FINAL_ITER] = it0 - 1;
                __hip_atomic_store(P.status + ST_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
    }
    if (it0 >= it1) return;
    T* const lds_res = (T*)smem;
    T* const v = lds_res + (size_t)rl * LQP_BLK;
    T* const yrow = v + Nps;
    T* const cvl = yrow + Nps;
    T* const part = cvl + Nps;
    T* const z = part + (size_t)NWV * Nps;
    T* const u = z + Nps;
    T* const ps = u + Nps;
    T* const lb = ps + Nps;
    T* const ub = lb + Nps;
    T* const D = ub + Nps;
    T* const xs = D + Nps;
    T* const sz = xs + Nps;                                  // snapshot of (z, u, x) at the last check
    T* const su = sz + Nps;
    T* const sx = su + Nps;
    T* const red = sx + Nps;
    int* const flags = (int*)(red + NWV * 8 + 8);             // [0] exchange timed out (sticky), [1] verdict of this iteration
    T* const Gl = (T*)(flags + 8);                            // equality block: G = K^-1 As^T, T = G S^-1 (m x Nps each)
    T* const Tl = Gl + (size_t)m * Nps;
    T* const Asl = Tl + (size_t)m * Nps;                      // the scaled equality rows (read at every check)
    T* const Sm = Asl + (size_t)m * Nps;
    T* const Si = Sm + m * m;
    T* const s0l = Si + m * m;
    T* const bs = s0l + m;
    T* const nus_l = bs + m;
    T* const snu = nus_l + m;

    VecView<T> V(P.vecs + (size_t)b * P.vstride, n, m);
    T* scal = P.scal + (size_t)b * SC_WORDS;
    const T* packed = P.packed + (size_t)b * packed_blocks(P.K) * LQP_BLK;
    unsigned long long* xq = P.xchg + (size_t)b * XCHG_WORDS;
    const T rho = scal[SC_RHO];
    const T pnorm = scal[SC_PNORM];

    SplitResident<NT> rr;
    // (one instantiation of the block helpers per part: which blocks a workgroup holds is a compile-time fact)
#define LQP_BY_PART(CALL)                                                                   \
    do {                                                                                    \
        if (part_id == 0) { constexpr int PARTC = 0; CALL; }                                \
        else if (part_id == 1) { constexpr int PARTC = 1; CALL; }                           \
        else if constexpr (NP > 2) {                                                        \
            if (part_id == 2) { constexpr int PARTC = 2; CALL; }                            \
            else { constexpr int PARTC = 3; CALL; }                                         \
        }                                                                                   \
    } while (0)
    LQP_BY_PART((split_resident_load<KS, PARTC, NT, NP>(rr, lds_res, packed)));
    for (int i = tid; i < Nps; i += NT) {
        const bool in = i < n;
        z[i] = in ? V.z[i] : T(0); u[i] = in ? V.u[i] : T(0); ps[i] = in ? V.ps[i] : T(0);
        lb[i] = in ? V.lbs[i] : T(0); ub[i] = in ? V.ubs[i] : T(0); D[i] = in ? V.D[i] : T(1);
        cvl[i] = (in && m > 0) ? V.cv[i] : T(0);
        yrow[i] = T(0);                                       // rows / columns of the partner stay zero
    }
    for (int r = tid; r < m; r += NT) bs[r] = V.bs[r];
    typename TERM::template Regs<T> tr;
    if constexpr (TERM::kind != 0) {
        static_assert(NT >= KS * LQP_NB, "the step with a term: one element per thread");
        if (tid < n) tr.load(P.termv + (size_t)b * term_stride<TERM>(n), n, tid, rho);
    }
    for (int i = tid; i < m * Nps; i += NT) { const int q = i / Nps, e = i - q * Nps; Asl[i] = e < n ? V.As[(size_t)q * n + e] : T(0); }
    for (int i = tid; i < NWV * Nps; i += NT) part[i] = T(0);
    if (tid < 8) flags[tid] = 0;
    // Which XCD are the workgroups of this QP on?  Each announces its id (write-through store, at once) and reads the
    // others' here, a whole load phase later.  On ONE XCD its L2 is their point of coherence: the granules are then stored
    // with workgroup scope (they stay in that L2; an sc1 store drops the line and the reader goes to memory for it) and
    // read as before (sc1 loads bypass the reader's L1 only).  Placement is the dispatcher's: never assumed, always asked.
    unsigned long long* const xcw = P.xchg + (size_t)P.B * XCHG_WORDS + (size_t)XCHG_TAIL * b + 8;
    const unsigned int xcd_me = my_xcd();
    // (tagged with the launch's first iteration: a problem sees one launch of this kernel per check segment when the batch takes
    //  turns on the chip, and the dispatcher is free to place every one of them differently)
    const unsigned long long ann = (unsigned long long)(it0 + 1) << 16;
    if (tid == 0) __hip_atomic_store(xcw + part_id, ann | 0x100ull | xcd_me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid == 0) {
        int same = P.xcd_local;
        for (int pp = 0; pp < NP && same; ++pp) {
            if (pp == part_id) continue;
            unsigned long long g = 0;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            while (((g = __hip_atomic_load(xcw + pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & ~0xFFFFull) != ann) {
                __builtin_amdgcn_s_sleep(2);
                if (__builtin_amdgcn_s_memrealtime() - t0 > 50000000ULL) { g = ~0ull; break; }      // (0.5 s: the exchange below will flag it)
            }
            same = (unsigned int)(g & 0xFFull) == xcd_me;
        }
        flags[2] = same;
    }
    __syncthreads();
    const bool xlocal = flags[2] != 0;
    auto xstore = [&](unsigned long long* ptr, const unsigned long long val) {
        if (xlocal) __hip_atomic_store(ptr, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_store(ptr, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    // ---- equality constraints: H <- H + T G^T with G = K^-1 As^T, S = As G, T = G S^-1 (what wg_eq_correct does to the
    //      blocks in global memory, three passes over them in a launch of its own) applied to the blocks in REGISTERS:
    //      m products with the blocks this kernel holds anyway, the partner's half through the exchange granules.  The
    //      corrected blocks only go back to global memory if a continuation launch needs them (end of the kernel). ----
    const bool eq_here = m > 0 && P.eq_in_loop;
    const int moff = eq_here ? m : 0;                         // the iterations' exchanges follow these m in buffer parity
    if (m > 0 && !eq_here) {
        for (int i = tid; i < m * Nps; i += NT) { const int q = i / Nps, e = i - q * Nps; Tl[i] = e < n ? V.Tm[(size_t)q * n + e] : T(0); }
        for (int r = tid; r < m; r += NT) s0l[r] = V.s0[r];
    }
    if (eq_here) {
        if (part_id == 0 && tid == 0 && P.info[b] != 0) P.status[ST_NOTSPD] = 1;      // (k_spd_end did not run)
        for (int q = 0; q < m; ++q) {
            LQP_BY_PART((wg_sym_gemv_split<KS, PARTC, NT, NP>(rr, lds_res, Nps, Asl + (size_t)q * Nps, yrow, part)));
            wg_barrier_lds();
            if (tid < Nps) {
                const int i = tid;
                const T own = split_combine<NT>(i, Nps, yrow, part);
                const unsigned int tag = 0x20000000u + (unsigned int)q;
                unsigned long long* base = xq + (size_t)(q & 1) * XPAR;
                xstore(base + (size_t)part_id * XPART + i,
                       ((unsigned long long)tag << 32) | (unsigned long long)__builtin_bit_cast(unsigned int, own));
                T y = T(0);
#pragma unroll
                for (int pp = 0; pp < NP; ++pp) {                 // same order on every workgroup
                    T term = own;
                    if (pp != part_id) {
                        const unsigned long long* src = base + (size_t)pp * XPART + i;
                        unsigned long long g = 0;
                        if (!flags[0]) {
                            unsigned int spins = 0;
                            unsigned long long t0 = 0;
                            for (;;) {
                                g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (((unsigned int)(g >> 32) & 0x3FFFFFFFu) == tag) break;
                                if ((++spins & 1023u) == 0) {
                                    const unsigned long long now = __builtin_amdgcn_s_memrealtime();     // 100 MHz
                                    if (t0 == 0) t0 = now;
                                    else if (now - t0 > 50000000ULL) {                                   // 0.5 s: give up
                                        __hip_atomic_store(P.status + ST_TIMEOUT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                        flags[0] = 1;
                                        break;
                                    }
                                }
                            }
                        }
                        term = __builtin_bit_cast(float, (unsigned int)g);
                    }
                    y = pp == 0 ? term : y + term;
                }
                Gl[(size_t)q * Nps + i] = -y;
            }
            wg_barrier_lds();
        }
        // S = As G (m x m), one wave per entry
        for (int t = w; t < m * m; t += NWV) {
            const int q = t / m, q2 = t - q * m;
            T acc = T(0);
            for (int i = lane; i < n; i += 64) acc += Asl[(size_t)q * Nps + i] * Gl[(size_t)q2 * Nps + i];
            acc = wave_sum(acc);
            if (lane == 0) Sm[t] = acc;
        }
        wg_barrier_lds();
        {                                                      // S^-1 by Gauss-Jordan (S is SPD: no pivoting), m <= 16
            const int bad = wg_gj_inverse_spd(Sm, Si, m, [] { wg_barrier_lds(); });
            if (bad && tid == 0) { if (P.info[b] == 0) P.info[b] = Ks * 64 + 1; P.status[ST_NOTSPD] = 1; }   // A rank deficient
        }
        wg_barrier_lds();
        // T = G S^-1, c = T b, s0 = S^-1 b (both workgroups hold them; the copies in global memory are for later launches)
        for (int t = tid; t < m * Nps; t += NT) {
            const int q = t / Nps, e = t - q * Nps;
            T acc = T(0);
            for (int q2 = 0; q2 < m; ++q2) acc += Gl[(size_t)q2 * Nps + e] * Si[q2 * m + q];
            Tl[t] = acc;
            if (part_id == 0 && e < n) V.Tm[(size_t)q * n + e] = acc;
        }
        for (int q = tid; q < m; q += NT) {
            T acc = T(0);
            for (int q2 = 0; q2 < m; ++q2) acc += Si[q * m + q2] * bs[q2];
            s0l[q] = acc;
            if (part_id == 0) V.s0[q] = acc;
        }
        wg_barrier_lds();
        for (int e = tid; e < Nps; e += NT) {
            T acc = T(0);
            for (int q = 0; q < m; ++q) acc += Tl[(size_t)q * Nps + e] * bs[q];
            cvl[e] = e < n ? acc : T(0);
            if (part_id == 0 && e < n) V.cv[e] = acc;
        }
        // the blocks: thread t holds EPT consecutive elements of row t / LPR of every block
        LQP_BY_PART((split_eq_update<KS, PARTC, NT, NP>(rr, lds_res, Gl, Tl, m, Nps)));
        wg_barrier_lds();
    }
    for (int i = tid; i < Nps; i += NT) v[i] = (i < n) ? -ps[i] + rho * (z[i] - u[i]) : T(0);
    wg_barrier_lds();

    int slot = ctr_base;
    bool pending = false;                                     // a check's verdict is still open (uniform)
    int pend_it = 0;
    const unsigned long long* pend_word = nullptr;
    unsigned long long dbt[6] = {0, 0, 0, 0, 0, 0}, dt0 = 0;  // debug: cycles of wave 0 (part 0) per phase
    const bool dbg_on = DBG && P.dbg != nullptr && part_id == 0;
    // 64-bit word {low: problems not optimal, high: arrivals} of a check -> 0 unknown, 1 all optimal, 2 go on
    auto verdict_of = [&](const unsigned long long cw) -> int {
        if ((unsigned int)(cw >> 32) < (unsigned int)P.B) return 0;
        return (unsigned int)cw == 0u ? 1 : 2;
    };
    auto wait_verdict = [&]() -> int {                        // (one thread) bounded spin, 2 s
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            const int vd = verdict_of(__hip_atomic_load(pend_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (vd) return vd;
            __builtin_amdgcn_s_sleep(4);
            if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ULL) {
                __hip_atomic_store(P.status + ST_TIMEOUT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return 1;
            }
        }
    };
    auto store_state = [&]() {                                // the iterate as it stands (part 0)
        for (int i = tid; i < n; i += NT) { V.z[i] = z[i]; V.u[i] = u[i]; V.x[i] = xs[i]; }
        for (int r = tid; r < m; r += NT) V.nu[r] = nus_l[r];
    };
    auto leave_with_snapshot = [&]() {                        // every problem was optimal at iteration pend_it
        if (blockIdx.x == 0 && tid == 0) {
            P.status[ST_FINAL_ITER] = pend_it;
            __hip_atomic_store(P.status + ST_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (part_id == 0) {
            for (int i = tid; i < n; i += NT) { V.z[i] = sz[i]; V.u[i] = su[i]; V.x[i] = sx[i]; }
            for (int r = tid; r < m; r += NT) V.nu[r] = snu[r];
        }
    };

    // One iteration.  COLD = std::true_type: a check iteration or the last one of the launch (nu, the six norms, the
    // counters, the snapshot, a blocking wait for an open verdict); std::false_type: everything else -- the hot
    // variant carries none of that code, and the hot iterations run in an inner loop of their own below, so the
    // register allocator keeps the resident blocks (and everything else the product needs) out of scratch there.
    // Returns 1 when the workgroup is done (all problems were optimal at the last check).
    // relax_tag: how the element-wise step takes control['alpha'] -- the hot loop exists once per value of P.relax (RelaxOff: the plain
    // step's loop, the code it was before the factor existed; RelaxOn), a cold iteration branches at run time (RelaxDyn)
    auto iterate = [&](auto cold_tag, auto relax_tag, const int it, const bool check) -> int {
        constexpr bool COLD = decltype(cold_tag)::value;
        if (dbg_on) dt0 = clock64();
        // ---- part 0: look at the open verdict while the product runs ----
        unsigned long long cw = 0;
        const bool look = !EACH && pending && part_id == 0 && tid == 0;
        if (look) cw = __hip_atomic_load(pend_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        LQP_BY_PART((wg_sym_gemv_split<KS, PARTC, NT, NP>(rr, lds_res, Nps, v, yrow, part)));
        if (look) {
            int vd = verdict_of(cw);
            if constexpr (COLD) { if (vd == 0) vd = wait_verdict(); }
            flags[1] = vd;
        }
        wg_barrier_lds();
        if (dbg_on) { const unsigned long long t = clock64(); dbt[0] += t - dt0; dt0 = t; }
        int verdict = (!EACH && pending && part_id == 0) ? flags[1] : 0;
        if constexpr (COLD) {
            if (m > 0) {                                      // nu = T^T w - s0 while v is still w
                for (int r = w; r < m; r += NWV) {
                    T acc = T(0);
                    for (int i = lane; i < n; i += 64) acc += Tl[(size_t)r * Nps + i] * v[i];
                    acc = wave_sum(acc);
                    if (lane == 0) nus_l[r] = acc - s0l[r];
                }
                wg_barrier_lds();
            }
        }
        T xi = T(0);
        if (tid < Nps) {
            const int i = tid;
            const T own = split_combine<NT>(i, Nps, yrow, part);
            // ---- exchange: publish this element's partial (part 0: with the verdict), fetch the partner's ----
            const unsigned int tag = (unsigned int)(it + 1);
            unsigned long long* base = xq + (size_t)((it + moff) & 1) * XPAR;
            xstore(base + (size_t)part_id * XPART + i,
                   ((unsigned long long)(tag | ((unsigned int)verdict << 30)) << 32) |
                       (unsigned long long)__builtin_bit_cast(unsigned int, own));
            if (dbg_on) { const unsigned long long t = clock64(); dbt[1] += t - dt0; dt0 = t; }
            T y = T(0);
#pragma unroll
            for (int pp = 0; pp < NP; ++pp) {                     // same order on every workgroup
                T term = own;
                if (pp != part_id) {
                    const unsigned long long* src = base + (size_t)pp * XPART + i;
                    unsigned long long g = 0;
                    if (!(verdict == 1 && part_id == 0) && !flags[0]) {      // (part 0 leaving: nothing to fetch)
                        unsigned int spins = 0;
                        unsigned long long t0 = 0;
                        for (;;) {
                            g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (((unsigned int)(g >> 32) & 0x3FFFFFFFu) == tag) break;
                            if ((++spins & 1023u) == 0) {
                                const unsigned long long now = __builtin_amdgcn_s_memrealtime();     // 100 MHz
                                if (t0 == 0) t0 = now;
                                else if (now - t0 > 50000000ULL) {                                   // 0.5 s: give up
                                    __hip_atomic_store(P.status + ST_TIMEOUT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    flags[0] = 1;
                                    break;
                                }
                            }
                        }
                    }
                    if (!EACH && pp == 0 && pending) {            // the verdict travels in part 0's tags
                        verdict = (int)((unsigned int)(g >> 62));
                        if (tid == 0) flags[1] = verdict;
                    }
                    term = __builtin_bit_cast(float, (unsigned int)g);
                }
                y = pp == 0 ? term : y + term;
            }
            if (dbg_on) { const unsigned long long t = clock64(); dbt[2] += t - dt0; dt0 = t; }
            xi = cvl[i] - y;
        }
        if (!EACH && pending) {
            // the verdict is uniform over both workgroups: part 0 read it before the exchange, part 1 found it in the tags
            if (part_id != 0) { wg_barrier_lds(); verdict = flags[1]; }
            if (verdict == 1) return 1;
            if (verdict == 2) pending = false;
        }
        T mx[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) mx[q] = T(0);
        T ia[4] = {T(0), T(0), T(0), T(0)};                   // (EACH, control['infeasible']: the certificate's terms, see infeas_view)
        T da[4] = {T(0), T(0), T(0), T(0)};                   // (... and the dual certificate's, control['unbounded'], see dinf_elem)
        InfeasView<T> isv = {nullptr, nullptr, n, false, 0};
        if constexpr (COLD && EACH) { if (check && P.snap) isv = infeas_view(P, b, it, rho); }
        if (tid < Nps) {
            const int i = tid;
            xs[i] = xi;
            const AdmmStep<T> sp = admm_step_term_tag<decltype(relax_tag), TERM>(P, xi, z[i], u[i], lb[i], ub[i], rho, tr);
            const T zn = sp.zn, un = sp.un;
            const bool in = i < n;
            if (in) { z[i] = zn; u[i] = un; }
            if constexpr (COLD) {
                if (check) {
                    if constexpr (!EACH) { sz[i] = zn; su[i] = un; sx[i] = xi; }      // snapshot for a late "all optimal"
                    if (in) {
                        T qx = v[i] - rho * xi;
                        for (int q = 0; q < m; ++q) qx -= Asl[(size_t)q * Nps + i] * nus_l[q];
                        admm_step_norms<false>(mx, sp, xi, D[i], rho, qx);
                        // (every workgroup of the problem stores the same values into the same slot, see snap_stride)
                        if constexpr (EACH) { if (P.snap) { infeas_elem(ia, isv, i, rho * un, qx + sp.s, lb[i], ub[i]); dinf_elem(da, isv, i, xi, qx, ps[i], lb[i], ub[i]); } }
                    }
                }
            }
            v[i] = in ? -ps[i] + rho * (zn - un) : T(0);     // next iteration's right-hand side
        }
        if (dbg_on) { const unsigned long long t = clock64(); dbt[3] += t - dt0; dt0 = t; }
        if constexpr (COLD) {
            if (check) {
                if constexpr (!EACH) { for (int r = tid; r < m; r += NT) snu[r] = nus_l[r]; }
                // six inf-norms: per wave by DPP, then ONE thread folds the 16 wave results
#pragma unroll
                for (int q = 0; q < 6; ++q) mx[q] = wave_max(mx[q]);
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < 6; ++q) red[w * 8 + q] = mx[q];
                }
                __syncthreads();
                T mv[6];                                       // (only the thread that folds them holds the norms)
                auto fold_norms = [&]() {
#pragma unroll
                    for (int q = 0; q < 6; ++q) mv[q] = red[q];
#pragma unroll 1
                    for (int ww = 1; ww < NWV; ++ww) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) mv[q] = tmax(mv[q], red[ww * 8 + q]);
                    }
                };
                if constexpr (EACH) {
                    if (tid == 0) {                           // (every workgroup of the problem: the very same numbers, the same verdict)
                        fold_norms();
                        const LoopCheck<T> ck = loop_check(P, mv, pnorm);
                        flags[4] = ck.solved ? 1 : 0;
                        if (part_id == 0) {
                            loop_check_store<true>(P, scal, ck, mv, it);
                            // not optimal: into the check's slot in every mode (k_check_done at the end of a host-driven chunk)
                            if (!ck.solved) atomicAdd(P.counters + (size_t)slot * CT_WORDS + CT_NOTOPT, 1u);
                        }
                    }
                    ++slot;
                    __syncthreads();
                    int why = flags[4];                       // 1: optimal
                    if (P.snap) {
                        const int flagged = infeas_finish<T, NT>(P, isv, ia, da, isv.xo != 0, nus_l, bs, it, rho, red);      // 2 / 3: primal / dual infeasible
                        if (!why) why = flagged;
                    }
                    if (why) {
                        // leave with the state of iteration `it`: the iterate first, then the words that say so
                        if (part_id == 0) {
                            store_state();
                            if (tid == 0) each_stop(P, b, it, why);
                        }
                        return 1;
                    }
                } else {
                    if (part_id == 0 && tid == 0) {               // (the partner computed the very same numbers)
                        fold_norms();
                        const LoopCheck<T> ck = loop_check(P, mv, pnorm);
                        unsigned int* ct = P.counters + (size_t)slot * CT_WORDS;
                        loop_check_store<false>(P, scal, ck, mv, it);
                        // NOT the ordered arrival of the blocking loops: these adds to WANTS / TRIG are not waited for before the
                        // arrival, while the hot_past reader below reads both words once it has seen B arrivals.  The four words of a
                        // slot share one 16-byte line; whether the ordered form (a round trip per check in the headline's loop) would
                        // cost time here has not been measured.
                        if (ck.wants) atomicAdd(ct + CT_WANTS, 1u);
                        if (ck.trig) atomicAdd(ct + CT_TRIG, 1u);
                        atomicAdd((unsigned long long*)ct, (1ull << 32) | (ck.solved ? 0ull : 1ull));   // {not optimal, arrival}
                    }
                    pend_word = (const unsigned long long*)(P.counters + (size_t)slot * CT_WORDS);
                    pend_it = it;
                    pending = !P.split_seg;        // (one launch per check segment: the verdict is the next launch's / k_check_done's)
                    ++slot;
                }
            }
        }
        if (dbg_on) { const unsigned long long t = clock64(); dbt[4] += t - dt0; dt0 = t; }
        wg_barrier_lds();
        if (dbg_on) { const unsigned long long t = clock64(); dbt[5] += t - dt0; }
        return 0;
    };

    int left = 0;
    int it = it0;
    for (; it < it1 && !left;) {
        if (!EACH && P.hot_past && P.adaptive_rho && it > it0 && it % P.ar_iter == 0 && it < P.ar_max) {
            // An iteration at which the reference may adapt rho (:237-246).  Whether anything changes is decided by the check
            // BEFORE it -- any(do_rho_update) and the ratio test, both over the whole batch: the counters of that check, complete
            // once every problem has arrived.  Nothing to update: run on in this kernel (a solve that never adapts rho stays on the
            // register-resident loop: 3 us per iteration instead of the continuation kernel's 14).  Otherwise leave; the
            // continuation launch takes over at this iteration (status[ST_RESUME]) and begins with the event.
            if (tid == 0) {
                const unsigned int* ce = P.counters + (size_t)(((it - 1) / P.check_solved) % P.ring) * CT_WORDS;
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                unsigned long long cw;
                while ((unsigned int)((cw = __hip_atomic_load((const unsigned long long*)ce, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) < (unsigned int)P.B) {
                    __builtin_amdgcn_s_sleep(4);
                    if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ULL) {      // 2 s: give up, results are flagged
                        __hip_atomic_store(P.status + ST_TIMEOUT, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                }
                const bool fire = (unsigned int)cw != 0u &&
                                  __hip_atomic_load(ce + CT_WANTS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0 &&
                                  __hip_atomic_load(ce + CT_TRIG, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0;
                flags[3] = fire ? 1 : 0;
            }
            __syncthreads();
            if (flags[3]) break;
        }
        const bool check = (it % P.check_solved) == 0;
        if (check || it + 1 == it1) {
            left = iterate(std::true_type(), RelaxDyn(), it, check);
            ++it;
        } else {
            int e = (it / P.check_solved + 1) * P.check_solved;      // next special iteration: a check or the last one
            if (e > it1 - 1) e = it1 - 1;
            if (P.relax) {
#pragma unroll 1
                for (; it < e; ++it) {
                    left = iterate(std::false_type(), RelaxOn(), it, false);
                    if (left) break;
                }
            } else {
#pragma unroll 1
                for (; it < e; ++it) {
                    left = iterate(std::false_type(), RelaxOff(), it, false);
                    if (left) break;
                }
            }
        }
    }
    if (left) {
        if constexpr (!EACH) leave_with_snapshot();
        if (dbg_on && tid == 0)
            for (int q = 0; q < 6; ++q) P.dbg[(size_t)b * 8 + q] += dbt[q];
        return;
    }
    if (dbg_on && tid == 0)
        for (int q = 0; q < 6; ++q) P.dbg[(size_t)b * 8 + q] += dbt[q];
    // ---- end of the launch: a verdict still open is for the state we hold (the check ran in the last iteration) ----
    if (!EACH && pending && blockIdx.x == 0 && tid == 0) {
        if (wait_verdict() == 1 && !__hip_atomic_load(P.status + ST_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            P.status[ST_FINAL_ITER] = pend_it;
            __hip_atomic_store(P.status + ST_DONE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!EACH && P.hot_past && blockIdx.x == 0 && tid == 0) P.status[ST_RESUME] = it;      // (where the continuation launch goes on)
    if (part_id == 0) {
        store_state();
        if constexpr (EACH) { if (tid == 0) P.pstat[(size_t)b * PS_WORDS + PS_FINAL] = it1 - 1; }      // (not optimal so far)
    }
    // the loop goes on in a continuation launch, which reads the blocks from global memory: there they still lack the
    // equality correction
    if (eq_here) {
        T* packed_w = P.packed + (size_t)b * packed_blocks(P.K) * LQP_BLK;
        LQP_BY_PART((split_resident_store<KS, PARTC, NT, NP>(rr, lds_res, packed_w)));
    }
#undef LQP_BY_PART
}
template <int KS, int NT, bool DBG, int NP, typename FORM>
__global__ __launch_bounds__(NT) void k_admm_loop_split(const FwdParams<float> P, const int it0, const int it1, const int ctr_base) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    admm_loop_split_body<KS, NT, DBG, NP, FORM>(P, it0, it1, ctr_base, smem);
}

}  // namespace lqp
