// C ABI of the MI355X box-QP ADMM layer: workspace carving, launch
// orchestration, status reporting.  See include/lqp_amd.h for the contract.
#include "../../include/lqp_amd.h"
#include "lqp_boxqp.hpp"
#include "lqp_unroll.hpp"
#ifdef LQP_SPLIT_BUILD
// split build (lqp_py_amd/_lib.py build_library, tools/gen_split_build.py): the kernel instances are compiled in the
// translation units csrc/split/lqp_tu_*.hip; here they are only declared
#include "split/lqp_extern.inc"
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <vector>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>

using namespace lqp;

namespace {

constexpr int kRing = 2048;          // per-check counter slots (a continuation launch holds kRing / 2 checks: 10 000 iterations at a check every 10 in ONE launch)
// pivoted LU: one panel row per thread to 1024 rows, two to 2048, four (float32, panels of 4 columns) to 4096 (k_lu_factor_big):
// what bounds it is the LDS that holds L21^T and U12 of a panel, 2 * PB * N elements
inline int max_rows(int dtype) { return dtype == LQP_F32 ? 4096 : 2048; }
constexpr size_t kAlign = 256;
constexpr int kSplitMaxB = 8192;     // two-workgroup loop: exchange granules (32 KB per problem) are carved for batches up to this

struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* p) : base((char*)p) {}
    template <typename U> U* take(size_t count) {
        off = (off + kAlign - 1) / kAlign * kAlign;
        U* r = base ? (U*)(base + off) : nullptr;
        off += count * sizeof(U);
        return r;
    }
};

#define HIP_OK(call)                                                      \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) {                                           \
            if (getenv("LQP_DEBUG")) fprintf(stderr, "[lqp] %s failed: %s\n", #call, hipGetErrorString(e_)); \
            return LQP_ERR_HIP;                                           \
        }                                                                 \
    } while (0)
// what the launches enqueued so far have left behind, as a status
inline int last_error() { return hipGetLastError() == hipSuccess ? LQP_OK : LQP_ERR_HIP; }
// a batch that leaves half the chip idle takes two workgroups (row slabs, halves of the tiles) per problem
inline int small_batch_split(const int B, const bool gate = true) { return (B <= 128 && gate) ? 2 : 1; }

// dynamic LDS above 64 KB needs an opt-in per kernel
std::mutex g_attr_mutex;
std::unordered_map<const void*, int> g_attr_set;
int ensure_lds(const void* fn, int bytes) {
    if (bytes > 160 * 1024) return LQP_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(g_attr_mutex);
    auto it = g_attr_set.find(fn);
    if (it != g_attr_set.end() && it->second >= bytes) return LQP_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return LQP_ERR_HIP;
    g_attr_set[fn] = bytes;
    return LQP_OK;
}

// Occupancy answers and CU counts do not change for a (kernel, block size, LDS) on a device: the runtime calls cost
// microseconds each and a forward used to make nine of them.
struct OccKey { const void* fn; int nt, lds, dev; bool operator==(const OccKey& o) const { return fn == o.fn && nt == o.nt && lds == o.lds && dev == o.dev; } };
struct OccHash { size_t operator()(const OccKey& k) const { return std::hash<const void*>()(k.fn) ^ ((size_t)k.nt * 1315423911u) ^ ((size_t)k.lds << 7) ^ (size_t)k.dev; } };
std::unordered_map<OccKey, int, OccHash> g_occ;
int g_cus[64];
bool current_device_cus(int* dev, int* cus) {
    if (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev >= 64) return false;
    std::lock_guard<std::mutex> lock(g_attr_mutex);
    if (g_cus[*dev] == 0 && hipDeviceGetAttribute(&g_cus[*dev], hipDeviceAttributeMultiprocessorCount, *dev) != hipSuccess) return false;
    *cus = g_cus[*dev];
    return true;
}
template <typename F> bool blocks_per_cu(int* per_cu, F fn, int nt, int lds, int dev) {
    const OccKey key{(const void*)fn, nt, lds, dev};
    {
        std::lock_guard<std::mutex> lock(g_attr_mutex);
        auto it = g_occ.find(key);
        if (it != g_occ.end()) { *per_cu = it->second; return true; }
    }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, nt, lds) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(g_attr_mutex);
    g_occ[key] = *per_cu;
    return true;
}

struct Device { int dev = 0, cus = 0; };      // the current device and its CU count (current_device_cus)
// `workgroups` of (fn, nt threads, lds bytes) resident at once: kernels whose workgroups wait for each other inside the launch need
// every one of them on the chip -- ask the occupancy calculator for THIS kernel (block size, registers, LDS), not just the CU
// count.  (workgroups = 0: the kernel can run at all; more than 160 KB of LDS: ensure_lds refuses.)
template <typename F> bool fits(const Device& d, F fn, const int nt, const int lds, const long long workgroups) {
    int per_cu = 0;
    return ensure_lds((const void*)fn, lds) == LQP_OK && blocks_per_cu(&per_cu, fn, nt, lds, d.dev) && per_cu >= 1 &&
           workgroups <= (long long)d.cus * per_cu;
}

// ---- optional per-kernel-class timing with HIP events on the launch stream ----
enum { PC_SETUP = 0, PC_LU, PC_PACK, PC_LOOP, PC_RHO, PC_EPILOGUE, PC_BWD_BUILD, PC_SOLVE, PC_BWD_EPILOGUE,
       PC_MISC, PC_LOOP_TAIL, PC_SPD_INV, PC_EQ_CORR, PC_BWD_CHOL, PC_UNROLL, PC_UNROLL_SCALE, PC_COUNT };
struct ProfRec { int cls; hipEvent_t a, b; };
std::mutex g_prof_mutex;
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
double g_prof_ms[PC_COUNT];
long long g_prof_n[PC_COUNT];

struct ProfScope {
    hipStream_t st; int cls; bool on; hipEvent_t a, b;
    ProfScope(hipStream_t s, int c) : st(s), cls(c), on(g_prof_on) {
        if (on) {
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            (void)hipEventRecord(a, st);
        }
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord(b, st);
            std::lock_guard<std::mutex> lock(g_prof_mutex);
            g_prof_recs.push_back({cls, a, b});
        }
    }
};

// (environment knobs are read once: a forward consults two dozen of them; tests that flip one do so in a fresh process
//  or through LQP_ENV_NOCACHE=1)
int env_int(const char* name, int dflt) {
    static const bool nocache = getenv("LQP_ENV_NOCACHE") != nullptr;
    if (nocache) { const char* s = getenv(name); return s ? atoi(s) : dflt; }
    static std::mutex m;
    static std::unordered_map<std::string, std::pair<bool, int>> cache;
    std::lock_guard<std::mutex> lock(m);
    auto it = cache.find(name);
    if (it == cache.end()) {
        const char* s = getenv(name);
        it = cache.emplace(name, std::make_pair(s != nullptr, s ? atoi(s) : 0)).first;
    }
    return it->second.first ? it->second.second : dflt;
}

// Every LQP_* environment switch that steers a schedule, read ONCE per process (tests that flip one run in a fresh process
// or set LQP_ENV_NOCACHE=1, which re-reads them at every use).  -1: not set, the library decides.
// X(field of struct Knobs, environment variable, default): the one list struct Knobs and read_knobs are generated from;
// docs/KNOBS.md documents every entry (tests/test_tier_table.py holds the two together).
#define LQP_KNOBS(X) \
    X(bwd_chol, "LQP_BWD_CHOL", 1) \
    X(bwd_early, "LQP_BWD_EARLY", 1) \
    X(bwd_full, "LQP_BWD_FULL", 0) \
    X(bwd_lookahead, "LQP_BWD_LOOKAHEAD", 1) \
    X(inv_xcd, "LQP_INV_XCD", 1)                      /* the inverse's column tiles of one problem on one XCD (0: grid order) */ \
    X(dbg_lu2_absent, "LQP_DBG_LU2_ABSENT", 0)        /* tests only -- the partner workgroups of the two-workgroup LU are not launched */ \
    X(dbg_loop_absent, "LQP_DBG_LOOP_ABSENT", 0)      /* tests only -- bit 0 ... of the two-workgroup loop, bit 1 ... of the resident sweep, bit 2 ... of the unroll sweep, bit 3 ... of the two-workgroup streaming loop */ \
    X(bwd_refine, "LQP_BWD_REFINE", 1) \
    X(dbg_qpass, "LQP_DBG_QPASS", 0) \
    X(dbg_setup, "LQP_DBG_SETUP", 0) \
    X(epi_slabs, "LQP_EPI_SLABS", -1) \
    X(eq_in_loop, "LQP_EQ_IN_LOOP", 1) \
    X(launch_mode, "LQP_LAUNCH_MODE", 2) \
    X(linsolve, "LQP_LINSOLVE", 0) \
    X(loop512, "LQP_LOOP512", 0) \
    X(loop_dense, "LQP_LOOP_DENSE", 1) \
    X(loop_dense_w, "LQP_LOOP_DENSE_W", 1) \
    X(loop_small, "LQP_LOOP_SMALL", 1) \
    X(loop_split, "LQP_LOOP_SPLIT", 1) \
    X(loop_split4, "LQP_LOOP_SPLIT4", 1) \
    X(loop_np2, "LQP_LOOP_NP2", 1) \
    X(spd_big_fuse, "LQP_SPD_BIG_FUSE", 1) \
    X(spd_big_f16, "LQP_SPD_BIG_F16", 1) \
    X(loop_split_seg, "LQP_LOOP_SPLIT_SEG", 1) \
    X(lu2, "LQP_LU2", 1) \
    X(lu_wide, "LQP_LU_WIDE", 1) \
    X(unroll_split, "LQP_UNROLL_SPLIT", 1) \
    X(lu_wide_min, "LQP_LU_WIDE_MIN", 1024)           /* the wide LU above this many rows (experiments; default 1024) */ \
    X(lu_mfma, "LQP_LU_MFMA", 1) \
    X(lu_nt, "LQP_LU_NT", 0) \
    X(lu_pb, "LQP_LU_PB", 0) \
    X(nosync_max_events, "LQP_NOSYNC_MAX_EVENTS", 12) \
    X(prep_fused, "LQP_PREP_FUSED", 1) \
    X(prep_one, "LQP_PREP_ONE", 1) \
    X(qpass, "LQP_QPASS", 1) \
    X(qs_lazy, "LQP_QS_LAZY", 1) \
    X(resident, "LQP_RESIDENT", 1) \
    X(rho_late, "LQP_RHO_LATE", 1) \
    X(spd_big, "LQP_SPD_BIG", 1) \
    X(spd_ptasks, "LQP_SPD_PTASKS", 48) \
    X(spd_resident, "LQP_SPD_RESIDENT", 1) \
    X(spd_resident4, "LQP_SPD_RESIDENT4", 1) \
    X(hot_past, "LQP_HOT_PAST", 1)                    /* the persistent two-workgroup loop runs on past rho events that change nothing */ \
    X(hot_rounds, "LQP_HOT_ROUNDS", 2)                /* with a GIVEN rho, rounds of {rho update, gated refactorisation, hot loop again} enqueued behind the first hot launch */ \
    X(bwd_equil, "LQP_BWD_EQUIL", 1)                  /* power-of-two symmetric equilibration of the Cholesky backward's free-set block */ \
    X(bwd_f16, "LQP_BWD_F16", 1)                      /* the backward's look-ahead Cholesky with its tile products on the float16 pipe (with LQP_SPD_F16; backward='kkt' keeps float32 products) */ \
    X(spd_turns, "LQP_SPD_TURNS", 1)                  /* more matrices than half the CUs -> the resident sweep anyway, its pairs taking turns on the chip */ \
    X(spd_f16, "LQP_SPD_F16", 1)                      /* the resident sweep's panel products on the float16 matrix pipe (two-half operands); 0: float32 matrix instructions */ \
    X(spd_split, "LQP_SPD_SPLIT", -1) \
    X(spec_launches, "LQP_SPEC_LAUNCHES", 6) \
    X(split2, "LQP_SPLIT2", 1) \
    X(sym512, "LQP_SYM512", 0) \
    X(sync_plan, "LQP_SYNC_PLAN", 1) \
    X(tail_epilogue, "LQP_TAIL_EPILOGUE", 1) \
    X(xcd_local, "LQP_XCD_LOCAL", 1)
struct Knobs {
#define LQP_KNOB_FIELD(field, env, dflt) int field;
    LQP_KNOBS(LQP_KNOB_FIELD)
#undef LQP_KNOB_FIELD
    // LQP_PIV_COLS (default 1): the last pivot block of the backward's look-ahead Cholesky and of the resident sweep stops behind
    // the matrix's last real column (wg_pivot_block_mfma, COLS); 0: all 64 columns, the identity padding included.  Not in the list above: it selects no
    // schedule and changes no bit (tests/test_gpu_pivot_cols.py) -- it exists for the A/B timing.  docs/KNOBS.md, below its table.
    int piv_cols;
};
Knobs read_knobs() {
    Knobs k;
#define LQP_KNOB_READ(field, env, dflt) k.field = env_int(env, dflt);
    LQP_KNOBS(LQP_KNOB_READ)
#undef LQP_KNOB_READ
    k.piv_cols = env_int("LQP_PIV_COLS", 1);
    return k;
}
const Knobs& knobs() {
    static const bool nocache = getenv("LQP_ENV_NOCACHE") != nullptr;
    static const Knobs cached = read_knobs();
    if (!nocache) return cached;
    static thread_local Knobs fresh;
    fresh = read_knobs();
    return fresh;
}

// The LU kernels that share a matrix between workgroups (lqp_lu2.hpp, lqp_lu_wide.hpp) need all of them resident at once; the
// launch checks that they fit, not that the chip is otherwise idle (another stream's kernels, RCCL).  When a hand-off times out
// (info word -7: the waits are bounded, the kernels drain) the call is repeated ONCE with one workgroup per matrix (SoloScope).
thread_local bool t_single_wg_lu = false;
unsigned long long* g_lu_dbg = nullptr;     // optional device buffer (4 counters per problem), debug only
std::atomic<unsigned int> g_unroll_run{1u};     // launches of the two-workgroup unroll sweep so far: each one's hand-off words carry its number

// ---- LU launch: pick panel width / trailing-update flavour --------------------
template <typename T, int PB, bool MFMA, int NT>
int launch_lu_impl(hipStream_t st, int B, T* M, int N, int ld, size_t mstride, int* piv, int pstride, int* info,
                   const int* gate, const int* nvec) {
    const int lds = LuLds<T, PB>(round_up(N, 64)).total;
    auto fn = k_lu_factor<T, PB, MFMA, NT>;
    int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    { ProfScope ps(st, PC_LU);
      hipLaunchKernelGGL(fn, dim3(B), dim3(NT), lds, st, M, N, ld, mstride, piv, pstride, info, gate, knobs().dbg_setup ? nullptr : g_lu_dbg, nvec); }
    return last_error();
}

// N <= 512: 512 threads (one row per thread, 256-VGPR budget) -> 32-column panel for f32, 16 for f64;
// larger N: 1024 threads, 16 / 8 columns.  LQP_LU_PB / LQP_LU_MFMA / LQP_LU_NT override for experiments.
// 1024 < N <= 2048: two panel rows per thread (k_lu_factor_big)
template <typename T>
int launch_lu_big(hipStream_t st, T* M, int B, int N, int ld, size_t mstride, int* piv, int pstride, int* info,
                  const int* gate, const int* nvec) {
    if (N > (sizeof(T) == 4 ? 4096 : 2048)) return LQP_ERR_UNSUPPORTED;
    const int lds = N > 2048 ? LuLds<T, 4>(round_up(N, 64)).total : LuLds<T, lu_big_panel<T>()>(round_up(N, 64)).total;
    auto fn = k_lu_factor_big<T>;
    const int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    ProfScope ps(st, PC_LU);
    hipLaunchKernelGGL(fn, dim3(B), dim3(LQP_NT), lds, st, M, N, ld, mstride, piv, pstride, info, gate, nvec);
    return last_error();
}

// Two workgroups per matrix (lqp_lu2.hpp) when the batch leaves half the chip idle: N <= 512, at least three column blocks, 2 B
// workgroups resident (they wait for each other inside the launch), and the caller has 8 * LU2_SCR_WORDS bytes of scratch per
// problem (`scr`, problem b at scr + b * scr_stride words).  Returns -1: not applicable, take the one-workgroup kernel.
std::atomic<unsigned int> g_lu2_epoch{(unsigned int)std::chrono::steady_clock::now().time_since_epoch().count() | 1u};
template <typename T>
int launch_lu2(hipStream_t st, T* M, int B, int N, int ld, size_t mstride, int* piv, int pstride, int* info,
               const int* gate, const int* nvec, unsigned long long* scr, size_t scr_stride) {
    constexpr int PB = lu2_panel_width<T>();
    if (!scr || scr_stride < (size_t)LU2_SCR_WORDS || N > 512 || N < 3 * PB || knobs().lu2 == 0 || t_single_wg_lu) return -1;
    Device d;
    auto fn = k_lu_factor2<T, PB>;
    const int lds = Lu2Lds<T, PB>(round_up(N, 64)).total;
    if (!current_device_cus(&d.dev, &d.cus) || !fits(d, fn, LU2_NT, lds, shared_grid(B, 2))) return -1;
    const unsigned int epoch = g_lu2_epoch.fetch_add(1u) + 1u;
    { ProfScope ps(st, PC_LU);
      // (LQP_DBG_LU2_ABSENT: the hand-offs of workgroups b time out, info = -7, the caller repeats on one workgroup per matrix)
      hipLaunchKernelGGL(fn, dim3(knobs().dbg_lu2_absent ? B : shared_grid(B, 2)), dim3(LU2_NT), lds, st, M, N, ld, mstride, piv, pstride, info, gate, nvec, scr,
                         scr_stride, epoch, knobs().dbg_setup ? nullptr : g_lu_dbg, B, knobs().xcd_local != 0 ? 1 : 0); }
    return last_error();
}

// Several workgroups per matrix above 1024 rows (lqp_lu_wide.hpp) when the batch leaves most of the chip idle: W = what fits
// resident / B workgroups (>= 2) own the 128-byte column tiles cyclically.  `scr`: 4 * luw_scratch_words<T>(N) bytes per problem.
// Returns -1: not applicable, take the one-workgroup kernel.
template <typename T>
int launch_lu_wide(hipStream_t st, T* M, int B, int N, int ld, size_t mstride, int* piv, int pstride, int* info,
                   const int* gate, const int* nvec, unsigned long long* scr, size_t scr_stride) {
    const bool tall = N > 2048;          // float32 only: sixteen panel rows per thread, panels of 4 columns
    if (!scr || t_single_wg_lu || 2 * scr_stride < luw_scratch_words<T>(N) || N <= knobs().lu_wide_min || N > (sizeof(T) == 4 ? 4096 : 2048) ||
        knobs().lu_wide == 0 || (ld % 32) != 0 || (mstride % 32) != 0 || (((uintptr_t)M) % 128) != 0)
        return -1;
    int dev = 0, cus = 0, per_cu = 0;
    auto fn = k_lu_factor_wide<T>;
    if constexpr (sizeof(T) == 4) { if (tall) fn = k_lu_factor_wide_tall<T>; }
    const int lds = tall ? LuLds<T, 4>(round_up(N, 64)).total : LuLds<T, luw_pb<T>()>(round_up(N, 64)).total;
    if (!current_device_cus(&dev, &cus) || ensure_lds((const void*)fn, lds) != LQP_OK ||
        !blocks_per_cu(&per_cu, fn, LQP_NT, lds, dev) || per_cu < 1)
        return -1;
    int W = (cus * per_cu) / B;
    const int ntile = (N + luw_tw<T>() - 1) / luw_tw<T>();
    if (W > ntile) W = ntile;
    if (W > LUW_HDR - 2) W = LUW_HDR - 2;
    if (W < 2) return -1;
    const unsigned int epoch = g_lu2_epoch.fetch_add(1u) + 1u;
    { ProfScope ps(st, PC_LU);
      hipLaunchKernelGGL(fn, dim3(W * B), dim3(LQP_NT), lds, st, M, N, ld, mstride, piv, pstride, info, gate, nvec, (int*)scr,
                         2 * scr_stride, epoch, B, knobs().dbg_setup ? nullptr : g_lu_dbg); }
    return last_error();
}

template <typename T>
int launch_lu(hipStream_t st, T* M, int B, int N, int ld, size_t mstride, int* piv, int pstride, int* info,
              const int* gate, const int* nvec = nullptr, unsigned long long* scr = nullptr, size_t scr_stride = 0) {
    if (N > 512) {
        const int rw = launch_lu_wide<T>(st, M, B, N, ld, mstride, piv, pstride, info, gate, nvec, scr, scr_stride);
        if (rw >= 0) return rw;
    }
    if (N > 1024) return launch_lu_big<T>(st, M, B, N, ld, mstride, piv, pstride, info, gate, nvec);
    { const int r2 = launch_lu2<T>(st, M, B, N, ld, mstride, piv, pstride, info, gate, nvec, scr, scr_stride);
      if (r2 >= 0) return r2; }
    int nt = lu_threads<T>(N);
    int pb = lu_panel_width<T>(N);
#define LQP_LU_CASE(PBV, MF, NTV) return launch_lu_impl<T, PBV, MF, NTV>(st, B, M, N, ld, mstride, piv, pstride, info, gate, nvec)
    if constexpr (sizeof(T) == 4) {
        const int want_nt = knobs().lu_nt;
        if (want_nt == 1024) { nt = 1024; pb = std::min(pb, 16); }
        const int want = knobs().lu_pb;
        if ((want == 8 || want == 16 || (want == 32 && nt == 512)) && 2 * want * round_up(N, 64) * 4 <= 128 * 1024) pb = want;
        const bool mfma = knobs().lu_mfma != 0;
        if (nt == 512) {
            if (pb == 32) { if (mfma) LQP_LU_CASE(32, true, 512); LQP_LU_CASE(32, false, 512); }
            if (pb == 16) { if (mfma) LQP_LU_CASE(16, true, 512); LQP_LU_CASE(16, false, 512); }
            LQP_LU_CASE(8, false, 512);
        }
        if (pb == 16) { if (mfma) LQP_LU_CASE(16, true, 1024); LQP_LU_CASE(16, false, 1024); }
        LQP_LU_CASE(8, false, 1024);
    } else {
        if (nt == 512) {
            if (pb == 16) LQP_LU_CASE(16, true, 512);
            LQP_LU_CASE(8, true, 512);
        }
        if (pb == 16) LQP_LU_CASE(16, true, 1024);
        LQP_LU_CASE(8, true, 1024);
    }
#undef LQP_LU_CASE
}

template <typename T>
int launch_pack(hipStream_t st, int B, const T* LU, int N, int ld, size_t mstride, const int* piv, int pstride,
                T* packed, int* dest, const int* gate, const int* nvec = nullptr) {
    const int K = round_up(N, LQP_NB) / LQP_NB;
    const int lds = pack_lds_bytes<T>();
    auto fn = k_pack<T>;
    int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    const bool vec_ok = (ld % 4 == 0) && (mstride % 4 == 0) && (((uintptr_t)LU) % (4 * sizeof(T)) == 0);
    ProfScope ps(st, PC_PACK);
    hipLaunchKernelGGL(fn, dim3(B, small_batch_split(B, knobs().split2 != 0)), dim3(LQP_NT), lds, st, LU, N, ld, mstride, piv, pstride, packed,
                       packed_blocks(K) * LQP_BLK, dest, K * LQP_NB, vec_ok ? 1 : 0, gate, nvec);
    return last_error();
}

template <typename T>
int launch_solve(hipStream_t st, int B, const T* packed, int N, const int* dest, T* rhs, int nrhs, size_t bstride,
                 int rstride, int cstride, const int* nvec = nullptr) {
    const int K = round_up(N, LQP_NB) / LQP_NB, Np = K * LQP_NB;
    const int lds = solve_lds_bytes<T>(Np);
    auto fn = k_packed_solve<T>;
    int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    ProfScope ps(st, PC_SOLVE);
    hipLaunchKernelGGL(fn, dim3(B), dim3(LQP_NT), lds, st, packed, N, Np, K, dest, rhs, nrhs, bstride, rstride, cstride, nvec);
    return last_error();
}

// X = M^-1 from the packed factor (lqp_dense.hpp): G workgroups per matrix, each takes column tiles g, g + G, ...
template <typename T, bool SMALL>
int launch_lu_inverse_cfg(hipStream_t st, int B, int N, const T* packed, size_t pkstride, const int* dest, int dstride, T* X,
                          size_t xstride, int ldx, const int* gate) {
    typedef InvCfg<T, SMALL> C;
    const int Np = round_up(N, LQP_NB);
    const int lds = lu_inverse_lds_bytes<T, SMALL>(Np);
    if (lds > 160 * 1024) return LQP_ERR_UNSUPPORTED;
    auto fn = k_lu_inverse<T, SMALL>;
    const int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    int dev = 0, cus = 256;
    (void)current_device_cus(&dev, &cus);
    const int ntiles = (N + C::TWG - 1) / C::TWG;
    // (column tiles are independent: every tile its own workgroup while the grid stays within a few waves of workgroups per CU --
    //  several 256-thread workgroups per CU hide each other's barriers and operand loads)
    int G = std::max(1, std::min(ntiles, (12 * cus) / std::max(B, 1)));
    ProfScope ps(st, PC_PACK);
    // (the tiles of a problem side by side on one XCD -- they all read the same factor --, see k_lu_inverse)
    if (G > 1 && G < 65536 && B < 32768 && knobs().inv_xcd != 0)
        hipLaunchKernelGGL(fn, dim3(8 * ((B + 7) / 8) * G), dim3(256), lds, st, packed, pkstride, N, G | (B << 16), dest, dstride, X, xstride,
                           ldx, gate);
    else
        hipLaunchKernelGGL(fn, dim3(B, G), dim3(256), lds, st, packed, pkstride, N, 0, dest, dstride, X, xstride, ldx, gate);
    return last_error();
}
// float32: 64-column tiles on v_mfma_f32_32x32x2 while Y fits the LDS (N <= 576), 16-column tiles on v_mfma_f32_16x16x4 above
template <typename T>
int launch_lu_inverse(hipStream_t st, int B, int N, const T* packed, size_t pkstride, const int* dest, int dstride, T* X,
                      size_t xstride, int ldx, const int* gate) {
    if constexpr (sizeof(T) == 4) {
        if (lu_inverse_lds_bytes<T, false>(round_up(N, LQP_NB)) > 160 * 1024)
            return launch_lu_inverse_cfg<T, true>(st, B, N, packed, pkstride, dest, dstride, X, xstride, ldx, gate);
    }
    return launch_lu_inverse_cfg<T, false>(st, B, N, packed, pkstride, dest, dstride, X, xstride, ldx, gate);
}
template <typename T> inline bool lu_inverse_fits(int Np) {
    return lu_inverse_lds_bytes<T, false>(Np) <= 160 * 1024 || (sizeof(T) == 4 && lu_inverse_lds_bytes<T, true>(Np) <= 160 * 1024);
}

// first failing batch index from the per-problem info array (host side, after a sync)
// host_info: the same words in pinned host memory, stored there by the last kernel the stream has run (host_report): the
// stream is waited for, nothing is copied
int first_failure(hipStream_t st, const int* info_dev, int B, int* fail_index, const int* host_info = nullptr) {
    std::vector<int> h;
    const int* words = host_info;
    if (host_info) {
        HIP_OK(hipStreamSynchronize(st));
    } else {
        h.resize(B);
        HIP_OK(hipMemcpyAsync(h.data(), info_dev, sizeof(int) * B, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        words = h.data();
    }
    *fail_index = -1;
    for (int i = 0; i < B; ++i)
        if (((const volatile int*)words)[i] == -7) { *fail_index = i; return LQP_ERR_TIMEOUT; }      // a multi-workgroup LU never met its partner
    for (int i = 0; i < B; ++i)
        if (((const volatile int*)words)[i] != 0) { *fail_index = i; return LQP_ERR_SINGULAR; }
    return LQP_OK;
}


// A synchronous call waits for its report, not for its stream: the words of a host report (pinned host memory, all set to
// -1 by the call before its first launch; no word the kernels store is -1) are polled until none is missing.  A
// hipStreamSynchronize of a ~0.5 ms schedule parks the thread after 100 us of spinning and pays the interrupt + wake-up
// on top of the completion signal's trip; the polled word is seen ~a microsecond after the store.  The device results
// themselves are stream-ordered like those of any torch operator -- the host only ever reads the report.  The stream is
// queried every ~50 us of waiting: a drained (or failed) stream whose report is still incomplete is an error, not a hang.
void report_reset(int* host_report, int words) {
    for (int i = 0; i < words; ++i) ((volatile int*)host_report)[i] = -1;
}
int wait_report(hipStream_t st, const int* host_report, int words) {
    const volatile int* r = (const volatile int*)host_report;
    int first_missing = 0;
    auto t_query = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        while (first_missing < words && r[first_missing] != -1) ++first_missing;      // (-7, a hand-off that timed out, HAS arrived)
        if (first_missing >= words) { std::atomic_thread_fence(std::memory_order_acquire); return LQP_OK; }
        __builtin_ia32_pause();
        if ((spins & 255u) == 255u) {
            const auto now = std::chrono::steady_clock::now();
            if (now - t_query > std::chrono::microseconds(50)) {
                t_query = now;
                const hipError_t q = hipStreamQuery(st);
                if (q == hipSuccess) {              // everything enqueued has run: the report must be complete now
                    for (int i = first_missing; i < words; ++i) if (r[i] == -1) return LQP_ERR_HIP;
                    return LQP_OK;
                }
                if (q != hipErrorNotReady) return LQP_ERR_HIP;
            }
        }
    }
}

// What a synchronous forward does once its whole schedule is enqueued: wait for the report (wait_report, when it sits in
// the caller's pinned memory), look at the info / flag words of every problem, fill the statistics.  `stats` comes in
// with n_launch / linsolve_used / factor_launches / loop_workgroups of the enqueue and keeps them.
// LQP_RETRY_LU (internal): the matrix left the symmetric x-update -- repeat the solve with linsolve = 1.
constexpr int LQP_RETRY_LU = 100;
// the solve's own figures, from the status block it left (`rv`: a host copy, or the words in pinned host memory)
inline void solve_stats(lqp_boxqp_stats* stats, const volatile int* rv, const int max_iters, const int check) {
    const int final_iter = rv[ST_DONE] ? rv[ST_FINAL_ITER] : max_iters - 1;
    stats->iters = final_iter;
    stats->n_factor = 1 + rv[ST_NFACTOR];
    stats->n_solve = final_iter + 1;
    stats->n_check = final_iter / check + 1;
    stats->rho_updated = rv[ST_RHO_UPDATED];
    stats->fail_index = -1;
    stats->any_lb = rv[ST_ANY_LB]; stats->any_ub = rv[ST_ANY_UB];
}
inline bool flags_timeout_loop(const int* rep) { return ((const volatile int*)rep)[ST_TIMEOUT] != 0; }
// the run-time twins of the Term traits (lqp_boxqp.hpp), by Term*::kind
constexpr int kTerms = 6;
constexpr int kTermSlots[kTerms] = {TermNone::slots, TermL1::slots, TermSoft::slots, TermLog::slots, TermPwl::slots, TermHuber::slots};
constexpr int kTermInputs[kTerms] = {TermNone::n_in, TermL1::n_in, TermSoft::n_in, TermLog::n_in, TermPwl::n_in, TermHuber::n_in};
constexpr int kTermFlag[kTerms] ={TermNone::input_flag, TermL1::input_flag, TermSoft::input_flag, TermLog::input_flag, TermPwl::input_flag, TermHuber::input_flag};
int collect_report(hipStream_t st, const int* rep, const bool polled, const int B, const int max_iters, const int check,
                   lqp_boxqp_stats* stats) {
    if (polled) {
        const int rc = wait_report(st, rep, ST_WORDS + 2 * B);
        if (rc) return rc;
    }
    const volatile int* rv = (const volatile int*)rep;
    int fail_index = -1, flags_or = 0;
    bool lu_timeout = false;
    for (int i = 0; i < B; ++i) {
        if (fail_index < 0 && rv[ST_WORDS + i] != 0) fail_index = i;
        lu_timeout = lu_timeout || rv[ST_WORDS + i] == -7;          // (a multi-workgroup LU never met its partner)
        flags_or |= rv[ST_WORDS + B + i];
    }
    for (int k = 1; k < kTerms; ++k) {
        if (!(flags_or & kTermFlag[k])) continue;
        // a solve with a separable term: what k_term_setup flags (a weight that is negative or not finite, a rho that is not positive ...).
        // First: what such data do to a factorisation (a negative rho leaves the symmetric x-update, a NaN makes a zero pivot) is no
        // finding of its own
        memset(stats, 0, sizeof(*stats));
        stats->fail_index = -1;
        for (int i = 0; i < B && stats->fail_index < 0; ++i) if (rv[ST_WORDS + B + i] & kTermFlag[k]) stats->fail_index = i;
        return LQP_ERR_INVALID;
    }
    if (lu_timeout && stats->linsolve_used != 2) return LQP_ERR_TIMEOUT;
    if (fail_index >= 0 && stats->linsolve_used == 2) return LQP_RETRY_LU;
    if (fail_index >= 0) {
        memset(stats, 0, sizeof(*stats));
        stats->fail_index = fail_index;
        return LQP_ERR_SINGULAR;
    }
    if (rv[ST_TIMEOUT] || (flags_or & RP_TIMEOUT)) return LQP_ERR_TIMEOUT;
    solve_stats(stats, rv, max_iters, check);
    stats->mode_used = 2;
    return LQP_OK;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// The form of a solve's loop kernels, derived ONCE (loop_form): the run-time twin of the Form tags (lqp_boxqp.hpp).  Every loop family
// has an instance per form it supports (family_has_form), and nothing but its selector below chooses one.
// The batch stops as one | control['stop'] = 'each': every problem stops and adapts rho as a batch of one (P.pstat) | ... with the primal
// infeasibility certificate in its check (control['infeasible']: P.snap) | ... and the dual one beside it (control['unbounded']:
// P.eps_dinf > 0) | the step with a separable term, one form per term (lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber: P.term, whose area shares its
// storage with the snapshots; the batch stops as one)
enum LoopForm { FORM_ALL, FORM_EACH, FORM_DETECT, FORM_CERTIFY, FORM_L1, FORM_SOFT, FORM_LOG, FORM_PWL, FORM_HUBER };
inline int form_term(const LoopForm form) { return form >= FORM_L1 ? form - FORM_L1 + 1 : 0; }      // (Term*::kind of the form, 0: none)
inline LoopForm loop_form(const int term, const bool each, const bool snapshots, const bool dual) {
    return term ? (LoopForm)(FORM_L1 + term - 1) : !each ? FORM_ALL : !snapshots ? FORM_EACH : dual ? FORM_CERTIFY : FORM_DETECT;
}
inline bool form_each(const LoopForm form) { return form == FORM_EACH || form == FORM_DETECT || form == FORM_CERTIFY; }
inline bool form_snapshots(const LoopForm form) { return form == FORM_DETECT || form == FORM_CERTIFY; }
template <typename T> LoopForm loop_form(const FwdParams<T>& P) { return loop_form(P.term, P.pstat != nullptr, P.snap != nullptr, P.eps_dinf > 0); }
template <typename F> auto by_form(const LoopForm form, F f) -> decltype(f(FormAll())) {
    switch (form) {
        case FORM_EACH:    return f(FormEach());
        case FORM_DETECT:  return f(FormDetect());
        case FORM_CERTIFY: return f(FormCertify());
        case FORM_L1:      return f(FormL1());
        case FORM_SOFT:    return f(FormSoft());
        case FORM_LOG:     return f(FormLog());
        case FORM_PWL:     return f(FormPwl());
        case FORM_HUBER:   return f(FormHuber());
        default:           return f(FormAll());
    }
}
template <typename T> struct FwdLayout {
    FwdParams<T> P;
    size_t bytes;
    unsigned int* vtrace_area;      // [kRing][2]: the check trace (FwdParams::vtrace points here when ctrl.reserved2 bit 2 asks for it)
    int* pstat_area;                // [B][PS_WORDS]: per-problem stopping (FwdParams::pstat points here when ctrl.reserved2 bit 3 asks for it)
    void* snap_area;                // [B][snap_stride]: the infeasibility certificate's snapshots, BEHIND `bytes` (lqp_boxqp_forward_detect alone)
    size_t detect_bytes;            // ... and the size that holds them
    size_t certify_bytes;           // ... and with the dual certificate's x and Qs x in every slot (lqp_boxqp_forward_certify; the same start)
    void* term_area;                // [B][term_stride<TERM>]: the area of a separable term, BEHIND `bytes` too (the same start: never together with the snapshots)
    size_t term_bytes[kTerms];      // ... and the size that holds it, by Term*::kind
    size_t bytes_for(const LoopForm form) const {      // the workspace a solve of this form needs
        return form_term(form) ? term_bytes[form_term(form)] : form == FORM_CERTIFY ? certify_bytes : form == FORM_DETECT ? detect_bytes : bytes;
    }
};
// the workspaces whose last forward ran with ctrl.reserved2 bit 3: lqp_boxqp_problem_iters is valid for these alone.  Host state keyed
// by ADDRESS: an entry goes when another forward runs on the address; memory that was freed and handed out again without a forward in
// between still counts as known (include/lqp_amd.h says so: the caller owns the workspace's lifetime)
std::mutex g_each_mu;
std::unordered_set<const void*> g_each_ws;
inline void each_ws_note(const void* ws, const bool each) {
    std::lock_guard<std::mutex> lk(g_each_mu);
    if (each) g_each_ws.insert(ws); else g_each_ws.erase(ws);
}
inline bool each_ws_known(const void* ws) {
    std::lock_guard<std::mutex> lk(g_each_mu);
    return g_each_ws.count(ws) != 0;
}

template <typename T>
FwdLayout<T> carve_forward(void* ws, int B, int n, int m) {
    FwdLayout<T> L;
    memset(&L.P, 0, sizeof(L.P));
    FwdParams<T>& P = L.P;
    P.B = B; P.n = n; P.m = m; P.N = n + m;
    P.Np = round_up(P.N, LQP_NB); P.K = P.Np / LQP_NB; P.ldq = round_up(n, 4);
    P.Ks = round_up(n, LQP_NB) / LQP_NB;
    P.vstride = vec_stride(n, m);
    Carver c(ws);
    P.status = c.take<int>(ST_WORDS);
    P.counters = c.take<unsigned int>((size_t)kRing * CT_WORDS);
    P.info = c.take<int>(B);            // (status | counters | info: one contiguous region for the deferred error fetch)
    P.bflags = c.take<int>(B);
    L.vtrace_area = c.take<unsigned int>((size_t)kRing * 2);      // (the check trace of verbose=True; in use: FwdParams::vtrace)
    P.scal = c.take<T>((size_t)B * SC_WORDS);
    P.vecs = c.take<T>((size_t)B * P.vstride);
    P.piv = c.take<int>((size_t)B * P.Np);
    P.dest = c.take<int>((size_t)B * P.Np);
    P.Qs = c.take<T>((size_t)B * n * P.ldq);
    P.M = c.take<T>((size_t)B * P.Np * P.Np);
    P.packed = c.take<T>((size_t)B * packed_blocks(P.K) * LQP_BLK);
    // granules of the two-workgroup loop (only ever used when 2 B workgroups fit the chip)
    // (only where a two-workgroup kernel can run at all: 32 KB per problem -- a batch of 8192 small problems used to carry 256 MB of it)
    // (above 512 rows: the streaming loop on two workgroups per problem, k_admm_loop_np2 -- batches that can leave half the chip idle)
    P.xchg = (sizeof(T) == 4 && P.Ks >= SPLIT_MINK && ((B <= kSplitMaxB && P.Ks <= SPD_MAXK) || (B <= 256 && P.Ks <= SPD_BIGK)))
                 ? c.take<unsigned long long>((size_t)B * (XCHG_WORDS + XCHG_TAIL)) : nullptr;
    // granules of the dense LU-tier loop (lqp_dense.hpp): batches that can leave half a chip idle, n <= 256
    // granules of the dense LU-tier loops: two workgroups per problem to n = 256; W workgroups per problem for small batches at any
    // n the inverse kernel takes (two parities x n elements x one or two words)
    P.dnx_words = (B <= 256 && n <= DENSE_NMAX && P.N <= 1024) ? DNX_WORDS
                : (B <= 64 && P.N <= 2048) ? (int)std::max((size_t)DNX_WORDS, densew_xchg_words<T>(n)) : 0;
    P.dnx = P.dnx_words ? c.take<unsigned long long>((size_t)B * P.dnx_words) : nullptr;
    L.pstat_area = c.take<int>((size_t)B * PS_WORDS);      // (behind everything that was there before ABI 14: no offset moved)
    L.bytes = c.off + kAlign;
    c.off = L.bytes;                // (nothing in front of it moves, and lqp_boxqp_forward_workspace_bytes says what it said)
    L.snap_area = c.take<T>((size_t)B * snap_stride(n, m));
    L.detect_bytes = c.off + kAlign;
    c.off = L.bytes;
    c.take<T>((size_t)B * snap_stride(n, m, true));
    L.certify_bytes = c.off + kAlign;
    c.off = L.bytes;
    L.term_bytes[0] = L.bytes;      // (TermNone: no area)
    for (int k = 1; k < kTerms; ++k) {      // (every term's area at the same start)
        c.off = L.bytes;
        L.term_area = c.take<T>((size_t)B * kTermSlots[k] * round_up(n, 8));
        L.term_bytes[k] = c.off + kAlign;
    }
    return L;
}

// ---- the tier plan: what one attempt at a forward solve will launch, decided before its first launch ----
inline int spd_prep_lds_bytes(const int Ks) { return (2 * 64 * SPD_LS + 2 * LQP_NW + 64 * Ks) * 4; }      // (k_spd_prep)
typedef void (*SweepFn)(const FwdParams<float>, const int*);
typedef void (*SplitFn)(const FwdParams<float>, const int, const int, const int);
// the kernel of the first (hot) launch of the persistent mode
enum LoopKind {
    LOOP_ONE,           // k_admm_loop: one workgroup per problem
    LOOP_SPLIT,         // k_admm_loop_split: two (four) workgroups per problem, the matrix in their registers
    LOOP_SMALL,         // k_admm_loop_small: n <= 128, 256 threads per problem
    LOOP_NP2,           // k_admm_loop_np2: above 512 rows, the streaming loop on two workgroups per problem
    LOOP_DENSE,         // k_admm_loop_dense: LU tier, n <= 256, the explicit inverse in the registers of two workgroups
    LOOP_DENSE_W        // k_admm_loop_dense_w: LU tier, W workgroups per problem
};
// Which family runs which form -- the ONE place that says so.  A family without the form of a solve is not planned: its problems run
// the one-workgroup loop, which holds every form, size, dtype and m.
inline bool family_has_form(const LoopKind kind, const LoopForm form) {
    switch (kind) {
        case LOOP_ONE: case LOOP_SMALL: case LOOP_SPLIT: return true;      // (the split loop's FormEach serves FormDetect and FormCertify)
        case LOOP_NP2: return form == FORM_ALL || form == FORM_L1 || form == FORM_SOFT || form == FORM_LOG || form == FORM_PWL || form == FORM_HUBER;
        default: return form == FORM_ALL;                                  // (the dense tiers)
    }
}
// Ks -> f(the KS of its instance) on NP workgroups per problem: two have 3 .. 6 as they are; then 7; everything else is 8
template <int KS> using KsTag = std::integral_constant<int, KS>;
template <int NP, typename F> auto by_ks(const int Ks, F f) -> decltype(f(KsTag<8>())) {
    if constexpr (NP == 2) switch (Ks) { case 3: return f(KsTag<3>()); case 4: return f(KsTag<4>()); case 5: return f(KsTag<5>()); case 6: return f(KsTag<6>()); default: break; }
    return Ks == 7 ? f(KsTag<7>()) : f(KsTag<8>());
}
template <int NP> SweepFn spd_resident_fn(const int Ks, const bool f16) {
    return by_ks<NP>(Ks, [&](auto ks) -> SweepFn {
        if constexpr (LQP_PIV_MFMA != 0) if (f16) return k_spd_resident<decltype(ks)::value, NP, true>;
        return k_spd_resident<decltype(ks)::value, NP, false>;
    });
}
// the split loop (FormEach serves FormDetect and FormCertify: it takes the certificates from P.snap and P.eps_dinf itself)
// (the DBG instance is FormAll's alone: with the debug counters set -- lqp_debug_set_lu_counters -- any other form runs the same kernels
//  and records no split-loop phases)
template <int NP> SplitFn loop_split_fn(const LoopForm form, const int Ks, const bool dbg) {
    if constexpr (NP == 2) if (form == FORM_ALL && dbg && (Ks < 3 || Ks > 7)) return k_admm_loop_split<8, 512, true, 2, FormAll>;
    return by_form(form, [&](auto f) {
        using FORM = typename std::conditional<decltype(f)::detect, FormEach, decltype(f)>::type;
        return by_ks<NP>(Ks, [&](auto ks) -> SplitFn { return k_admm_loop_split<decltype(ks)::value, 512, false, NP, FORM>; });
    });
}
inline SplitFn small_loop_kernel(const LoopForm form) {
    return by_form(form, [](auto f) -> SplitFn { return k_admm_loop_small<decltype(f)>; });
}
// the one-workgroup loop, first launch and continuation (same code, own name), 1024 threads.  One column per (RES, SYM): float64 has
// the first alone, and the symmetric path keeps its blocks on chip whatever `resident` says
template <typename T> using LoopFn = void (*)(const FwdParams<T>, int, int, int, int, int);
template <typename T> struct LoopPair { LoopFn<T> hot, tail; };
template <typename T> LoopPair<T> loop_kernels(const LoopForm form, const bool resident, const bool sym) {
    return by_form(form, [&](auto f) -> LoopPair<T> {
        using FORM = decltype(f);
        if constexpr (sizeof(T) == 4) {
            if (sym) return {k_admm_loop<T, true, false, 1024, true, FORM>, k_admm_loop<T, true, true, 1024, true, FORM>};
            if (resident) return {k_admm_loop<T, true, false, 1024, false, FORM>, k_admm_loop<T, true, true, 1024, false, FORM>};
        }
        return {k_admm_loop<T, false, false, 1024, false, FORM>, k_admm_loop<T, false, true, 1024, false, FORM>};
    });
}
// the streaming loop on two workgroups per problem: no instance for a per-problem form -- null, never another form's kernel; its one
// caller asks family_has_form(LOOP_NP2, form) first
inline LoopFn<float> np2_kernel(const LoopForm form) {
    return by_form(form, [](auto f) -> LoopFn<float> {
        if constexpr (decltype(f)::each) return nullptr;
        else return k_admm_loop_np2<decltype(f)>;
    });
}
// the extra arguments of lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber: the term (Term*::kind), its input vectors, its two outputs
struct TermArgs { int kind = 0; const void* in[TERM_IN_MAX] = {}; void* aux = nullptr; void* u_box = nullptr; };

constexpr int kMaxChecksPerLaunch = kRing / 4;

template <typename T> struct FwdPlan {
    int retry = 0;                      // forward_impl's retry bits of this attempt
    bool solo = false;                  // (retry bit 2: nothing shared between workgroups)
    int dbg_loop_absent = 0;            // LQP_DBG_LOOP_ABSENT
    // x-update: the symmetric inverse (lqp_spd.hpp) or the pivoted LU of the KKT matrix
    bool spd = false;
    bool spd_split = false;             // SPD_NP workgroups per matrix
    bool spd_turns = false;             // ... more matrices than half the CUs: the pairs of the resident sweep take turns
    bool spd_big_split = false;         // above 512 rows: two workgroups per matrix, a launch per phase of a pivot step
    bool spd_resident = false;          // all pivot steps in one launch, the matrix in the registers of its rs_np workgroups
    int rs_np = SPD_NP;
    SweepFn rs_fn = nullptr;
    int spd_pivot_tasks = 0;
    bool rho_late_big = false;          // k_spd_rho_big turns the sums k_spd_begin leaves into rho
    bool fuse2 = false;                 // k_spd_big_step: two pivot steps per pass over the tiles
    int f16 = 0;                        // ... its flag bit for the float16 pipe (32 or 0)
    // the loop
    LoopKind kind = LOOP_ONE;
    int kind_lds = 0;                   // LDS of LOOP_SMALL / LOOP_DENSE / LOOP_DENSE_W
    SplitFn small_fn = nullptr;         // LOOP_SMALL
    LoopFn<float> np2_fn = nullptr;     // LOOP_NP2
    TermArgs term;                      // a form with a term: what k_term_setup reads and k_fwd_epilogue<T, TERM> (the epilogue of that form) writes
    int kind_wg = 1;                    // workgroups per problem of the hot launch
    int densew_tpr = 0;
    bool loop_split_seg = false;        // mode 1: k_admm_loop_split per check segment, its pairs taking turns on the chip
    LoopFn<T> loop_fn = nullptr; int loop_nt = 1024, loop_lds = 0;     // hot launch of LOOP_ONE, every launch of mode 1
    LoopFn<T> tail_fn = nullptr; int tail_lds = 0;                     // continuation launches (LQP_NT threads)
    SplitFn split_fn = nullptr; int split_nt = 512, split_lds = 0;  // LOOP_SPLIT and loop_split_seg
    int mode = 0;                       // 2: persistent loop kernel, 1: one launch per check segment
    LoopForm form = FORM_ALL;           // which instance of every loop family runs (loop_form)
    bool inkernel_refactor = false;     // the continuation kernel refactorises at its adaptive-rho events itself
    // the scheduler
    bool up_front = false;              // run_planned: the whole schedule enqueued before anything is waited for
    bool hot_past = false;
    int hot_rounds = 0;
    bool tail_epilogue = false;
    int spec_launches = 0;
    // what lqp_boxqp_stats reports of it
    int factor_launches = 0, loop_workgroups = 1;
};

// ---- x-update linear algebra: pivoted LU of the KKT matrix, or the symmetric inverse (lqp_spd.hpp) ----
template <typename T> int plan_xupdate(FwdParams<T>& P, const lqp_boxqp_ctrl* ctl, const Knobs& k, const Device& d, FwdPlan<T>& plan) {
    const int B = P.B, n = P.n, m = P.m;
    const bool force_lu = (plan.retry & 1) != 0, solo = plan.solo;
    bool spd = false;
    if constexpr (sizeof(T) == 4) {
        const int want = ctl->linsolve != 0 ? ctl->linsolve : k.linsolve;
        const bool rho_pos = !(ctl->rho_mode == 1 && !(ctl->rho_value > 0.0));
        // (512 < n <= 1024: the sweep parks its panel in the M area, see wg_spd_sweep_big)
        spd = !force_lu && want != 1 && rho_pos && P.Ks <= SPD_BIGK && m <= SPD_MAXM &&
              (P.Ks <= SPD_MAXK || ((size_t)P.Np * P.Np >= (size_t)P.Ks * LQP_BLK && k.spd_big));
        // the equality correction (G, T: 2 m rows of 64 Ks floats next to the product's scratch) and the loop's vectors must
        // fit the 160 KB of LDS: large n with many equality rows (n > 960 at m >= 8, ...) stays on the LU path
        spd = spd && spd_factor_lds_bytes(m, P.Ks) <= 160 * 1024 && sym_loop_lds_bytes(n, m, P.Ks, 0) <= 160 * 1024;
    }
    plan.spd = spd; P.spd = spd ? 1 : 0;
    // (the LU path too: its refactorisations form (D Q) D again from Q and the scaling vector -- assemble_kkt_rows -- instead of
    //  reading a stored copy the setup kernel would have to write: 128 MB per batch at n = 500)
    P.qs_lazy = k.qs_lazy ? 1 : 0;

    // symmetric path with fewer problems than half the CUs: share each matrix between SPD_NP workgroups
    const bool share = (k.spd_split < 0 ? (B * SPD_NP <= d.cus ? 1 : 0) : k.spd_split) != 0 && !solo;
    plan.spd_pivot_tasks = k.spd_ptasks;
    bool spd_split = spd && P.Ks >= 3 && P.Ks <= SPD_MAXK && share && (size_t)P.Np * P.Np >= 2 * 64 * SPD_LS;     // room for W, W^T in the M area
    // More matrices than half the CUs (BASELINE configs[4]: 1024 per GPU): the resident sweep all the same, its pairs taking turns
    // on the chip as the loop's do (FwdParams::split_seg) -- partners are neighbours in dispatch order on one XCD (shared_map), so a
    // workgroup that waits for its partner waits for a CU that a COMPLETE earlier pair is about to leave.  Round 4 measured this
    // form slower than the one-workgroup sweep (8 turns x 0.36 ms against 2.9 ms); with the panel products on the float16 pipe a
    // turn is 0.28 ms and needs no pass over Q in front (k_spd_prep: 0.44 ms at B = 1024).
    bool spd_turns = false;
#if LQP_PIV_MFMA
    if (spd && !spd_split && !solo && P.xchg && P.Ks >= SPLIT_MINK && P.Ks <= SPD_MAXK && k.spd_turns != 0 && k.spd_resident != 0 && k.spd_f16 != 0 &&
        k.spd_split != 0 && (size_t)P.Np * P.Np >= rs2_xb_floats(P.Ks) && (size_t)P.Np * P.Np >= 2 * 64 * SPD_LS && B * SPD_NP > d.cus)
        spd_turns = spd_split = true;
#endif
    const bool spd_big_split = spd && P.Ks > SPD_MAXK && share;
    // ... and, with the exchange buffer in the M area and the step flags behind the loop's granules, in ONE launch
    bool spd_resident = spd_split && P.xchg && P.Ks >= SPLIT_MINK && (size_t)P.Np * P.Np >= rs2_xb_floats(P.Ks) && k.spd_resident != 0;
    if constexpr (sizeof(T) == 4) {
        if (spd_resident) {
            // workgroups per matrix of the resident sweep: 2, or 4 for batches up to a quarter of the CUs
            const int rlds = rs_q_lds_bytes(P.Ks);     // (the look-ahead sweep's counters behind the flags, the scaling vector behind them)
            const bool f16 = k.spd_f16 != 0;
            bool ok = false;
#if LQP_PIV_MFMA
            if (P.Ks >= 7 && 4 * B <= d.cus && k.spd_resident4 != 0) {
                plan.rs_fn = spd_resident_fn<4>(P.Ks, f16);
                ok = fits(d, plan.rs_fn, RS_NT, rlds, shared_grid(B, 4));
                if (ok) plan.rs_np = 4;
            }
#endif
            if (!ok) {
                plan.rs_fn = spd_resident_fn<2>(P.Ks, f16);
                ok = fits(d, plan.rs_fn, RS_NT, rlds, spd_turns ? 0 : shared_grid(B, SPD_NP));
            }
            spd_resident = ok;
        }
    }
    if (spd_turns && !spd_resident) { spd_turns = false; spd_split = false; }      // (the one-workgroup sweep after all)
    plan.spd_split = spd_split; plan.spd_turns = spd_turns; plan.spd_big_split = spd_big_split; plan.spd_resident = spd_resident;
    // rho = ||Qs||_F / sqrt(n): the norm is summed by k_spd_begin, which reads all of Q anyway, and rho is added to the
    // diagonal by the resident sweep -- the setup kernel then makes one pass over Q instead of two
    P.piv_cols = k.piv_cols != 0 ? 1 : 0;
    P.rho_late = (spd_resident && (!P.scale || P.qs_lazy) && ctl->rho_mode == 0 && k.rho_late) ? 1 : 0;
    // ... and above 512 rows on two workgroups per matrix: the sums k_spd_begin leaves are turned into rho by k_spd_rho_big
    plan.rho_late_big = spd_big_split && !spd_resident && (!P.scale || P.qs_lazy) && ctl->rho_mode == 0 && k.rho_late != 0 && (size_t)P.Np * P.Np >= (size_t)(2 * P.Ks + 1) * LQP_BLK;
    if (plan.rho_late_big) P.rho_late = 1;
    // two pivot steps per pass over the tiles (wg_spd_sweep_big, phases bits 2 .. 4): pivot + Y of step k | its update on
    // block column k + 1 alone | pivot + Y' of step k + 1 | ONE read-modify-write of every other tile with both products
    plan.fuse2 = k.spd_big_fuse != 0 && (size_t)P.Np * P.Np >= (size_t)(2 * P.Ks + 1) * LQP_BLK;
    // ... its panel blocks as two-half operands, the update products on the float16 pipe (lqp_f16x2.hpp)
    plan.f16 = (plan.fuse2 && k.spd_big_f16 != 0) ? 32 : 0;
    // auto-scaling on: ONE pass over Q for the column maxima, the symmetry verdict and the (unscaled) blocks, in front of
    // the setup kernel (k_spd_prep); the resident sweep scales its tiles as it loads them and sums ||Qs||_F itself
    P.prep_fused = 0;
#if LQP_PIV_MFMA
    if constexpr (sizeof(T) == 4) {
        P.prep_fused = (spd_resident && P.scale && P.qs_lazy && (ctl->rho_mode != 0 || P.rho_late) && k.prep_fused) ? 1 : 0;
        // ... and the one-workgroup tier (more problems than half the CUs, n <= 512): k_spd_inverse scales the prepared
        // blocks, sums ||Qs||_F and adds rho itself (wg_spd_factor)
        if (!P.prep_fused && spd && !spd_split && !spd_big_split && P.Ks <= SPD_MAXK && P.scale && P.qs_lazy &&
            ctl->rho_mode != 2 && (size_t)n * P.ldq >= (size_t)SPD_NP * P.Ks * LQP_NB + 8 &&      // (k_spd_prep's scratch per
            k.prep_one)                                                                   //  problem lives in its Qs area)
            P.prep_fused = 2;
    }
    // ... or no pass in front at all: the resident sweep reads Q itself, straight into the registers that keep it
    if (P.prep_fused == 1 && (size_t)n * P.ldq >= (size_t)plan.rs_np * (64 * P.Ks + 2) && k.qpass) P.prep_fused = 3;
#endif
    // the LDS opt-ins of the prologue's and the factorisation's kernels (launch_lu and launch_pack see to their own)
    int rc = ensure_lds((const void*)k_fwd_setup<T>, setup_lds_bytes<T>(n));
    if constexpr (sizeof(T) == 4) {
        if (!rc && (P.prep_fused == 1 || P.prep_fused == 2)) rc = ensure_lds((const void*)k_spd_prep<>, spd_prep_lds_bytes(P.Ks));
        if (spd) {
            const int lds = spd_factor_lds_bytes(m, P.Ks);
            if (!rc) rc = ensure_lds((const void*)(P.Ks > SPD_MAXK ? k_spd_inverse<2> : k_spd_inverse<1>), lds);
            if (!rc && (spd_big_split || spd_split)) rc = ensure_lds((const void*)k_spd_begin<>, lds);
            if (!rc && spd_big_split) rc = ensure_lds((const void*)k_spd_big_step<>, lds);
            if (!rc && spd_split && !spd_big_split) rc = ensure_lds((const void*)k_spd_step<>, lds);
            if (!rc && (spd_big_split || spd_split)) rc = ensure_lds((const void*)k_spd_end<>, lds);
        }
    }
    return rc;
}

// ---- the loop kernels, and whether one persistent launch can hold all their workgroups ----
template <typename T> int plan_loop_kernels(FwdParams<T>& P, const lqp_boxqp_ctrl* ctl, const Knobs& k, const Device& d, FwdPlan<T>& plan) {
    const int B = P.B, n = P.n, m = P.m, check = P.check_solved;
    const bool spd = plan.spd, plain = plan.form == FORM_ALL;
    // hot (first) launch: optional 512-thread build (256 VGPRs per thread: 16 register-resident blocks instead
    // of 8).  Measured SLOWER at B=128 n=500 (2.03 ms vs 1.54 ms; 1.76 ms with a 6-deep ring and 4 spills):
    // 8 waves hide the per-block dependent chain worse than 16, which costs more than the 8 extra resident
    // blocks save.  Kept selectable (LQP_LOOP512=1) for re-measurement; continuation launches always use 1024.
    const bool resident = loop_resident_ok<1024>(P.K, sizeof(T)) && k.resident != 0 && loop_lds_bytes<T>(n, m, P.Np, true) <= 160 * 1024;
    // (the measurement-only 512-thread builds have the plain form alone)
    const bool hot512 = resident && loop_resident_ok<512>(P.K, sizeof(T)) && k.loop512 != 0 && plain;
    plan.loop_lds = loop_lds_bytes<T>(n, m, P.Np, resident); plan.loop_nt = hot512 ? 512 : 1024;
    const LoopPair<T> fns = loop_kernels<T>(plan.form, resident, spd);
    plan.loop_fn = fns.hot; plan.tail_fn = fns.tail;
    // the continuation kernel also runs LU + pack (in-kernel adaptive-rho refactor): LDS = max of the three
    // (above 1024 rows the LU kernel is the two-rows-per-thread one, launched on its own: refactorisations go through the
    //  separate gated kernels, and the continuation kernel's LDS does not have to hold an LU panel)
    // (float64 too since round 5: the pipelined schedule enqueues every possible event up front -- nine at the defaults -- and with
    //  separate gated kernels each one cost four launches that do nothing when the solve is over: rho update, LU, pack, tail)
    plan.inkernel_refactor = P.N <= 1024;
    if constexpr (sizeof(T) == 4) {
        if (hot512 && !spd) plan.loop_fn = k_admm_loop<T, true, false, 512, false, FormAll>;
        if (spd) {
            P.sym_rl = sym_resident_lds_blocks(n, m, P.Ks);
            plan.loop_lds = sym_loop_lds_bytes(n, m, P.Ks, P.sym_rl); plan.loop_nt = 1024;
            plan.tail_lds = std::max(plan.loop_lds, spd_factor_lds_bytes(m, P.Ks));      // the tail refactorises in-kernel
            // optional 512-thread first launch (8 elements per thread, 12 register-resident blocks).  Measured at
            // B=128 n=500: 0.96-0.99 ms with an 8-deep ring (26 spilled VGPRs), 0.87 ms with a 6-deep one, against
            // 0.885 ms for the 1024-thread kernel: neither the halved instruction count nor the fewer streamed
            // blocks show, the product is bound by the un-overlapped sum of its resident and streamed phases.
            if (k.sym512 && plain) {
                P.sym_rl_hot = sym_resident_lds_blocks(n, m, P.Ks, resident_regs<512>(), 8);
                plan.loop_lds = sym_loop_lds_bytes(n, m, P.Ks, P.sym_rl_hot, 8);
                plan.loop_nt = 512; plan.loop_fn = k_admm_loop<T, true, false, 512, true, FormAll>;
            }
        }
    }
    if (const int rc = ensure_lds((const void*)plan.loop_fn, plan.loop_lds)) return rc;
    if (!spd) {
        plan.tail_lds = plan.loop_lds;
        if (P.N <= 1024) plan.tail_lds = std::max({plan.tail_lds, LuLds<T, (sizeof(T) == 4 ? 16 : 8)>(round_up(P.N, 64)).total, (int)pack_lds_bytes<T>()});
    }
    if (const int rc = ensure_lds((const void*)plan.tail_fn, plan.tail_lds)) return rc;

    // ---- launch mode ----
    int mode = ctl->launch_mode;
    if (mode == 0) mode = k.launch_mode;            // auto: persistent when every workgroup is resident
    if (ctl->check_hook || plan.solo) mode = 1;          // the hook sits between the check segments | no grid barrier
    if (mode == 2) {
        // the grid barrier needs EVERY workgroup resident -- of the hot kernel and of the continuation kernel
        // (own block size and LDS footprint): take the smaller of the two answers
        int per_cu = 0, per_cu_tail = 0;
        if (!blocks_per_cu(&per_cu, plan.loop_fn, plan.loop_nt, plan.loop_lds, d.dev) || !blocks_per_cu(&per_cu_tail, plan.tail_fn, LQP_NT, plan.tail_lds, d.dev))
            return LQP_ERR_HIP;
        per_cu = std::min(per_cu, per_cu_tail);
        if (per_cu < 1 || B > d.cus * per_cu) mode = 1;     // not every workgroup resident: no grid barrier
        // More problems than half the CUs but all resident (128 < B <= 256 here): the persistent one-workgroup kernel streams
        // two thirds of its matrix per iteration, while pairs of the two-workgroup kernel, taking turns, hold theirs in
        // registers (split_seg below) -- one launch per check segment then beats the persistent launch (B = 256, n = 500: loop
        // 0.82 -> 0.42 ms, step 1.87 -> 1.60 ms; B = 192: 1.63 -> 1.51).  Only when the caller left the mode to the library.
        if constexpr (sizeof(T) == 4) {
            if (mode == 2 && ctl->launch_mode == 0 && k.launch_mode == 2 && spd && P.xchg && 2 * B > d.cus && P.Ks >= SPLIT_MINK && P.Ks <= SPD_MAXK &&
                check >= 4 && k.loop_split != 0 && k.loop_split_seg != 0 && !ctl->check_hook)
                mode = 1;
        }
    }
    plan.mode = mode;
    return LQP_OK;
}

// ---- the kernel of the hot launch (plan.kind) and of the check segments of mode 1 (plan.loop_split_seg) ----
template <typename T> void plan_hot_kind(FwdParams<T>& P, const lqp_boxqp_ctrl* ctl, const Knobs& k, const Device& d, FwdPlan<T>& plan) {
    const int B = P.B, n = P.n, m = P.m, check = P.check_solved, mode = plan.mode, retry = plan.retry;
    const bool spd = plan.spd, solo = plan.solo;
    const LoopForm form = plan.form;
    if constexpr (sizeof(T) == 4) {
        // two workgroups per QP for the first (hot) launch: symmetric path, persistent mode, 2 B workgroups resident
        if (spd && mode == 2 && P.xchg && P.Ks >= SPLIT_MINK && P.Ks <= SPD_MAXK && check >= 4 && k.loop_split != 0) {
            // 512 threads x 256 VGPRs: every block of the workgroup's half lives in registers.  (The 1024-thread
            // build -- 12 blocks in 128 VGPRs, 6 in LDS, 16 waves -- spills ~60 VGPRs into the hot loop and measured
            // 0.38 ms against 0.28 ms at B = 128, n = 500; the template still takes NT = 1024.)
            int loop_np = 1;
            // four workgroups per QP (one column pair each) when the batch leaves room for them: B <= #CUs / 4
            if (P.Ks >= 7 && 4 * B <= d.cus && k.loop_split4 != 0) {
                plan.split_lds = split_loop_lds_bytes<512, 4>(P.Ks, m);
                plan.split_fn = loop_split_fn<4>(form, P.Ks, false);
                if (fits(d, plan.split_fn, plan.split_nt, plan.split_lds, shared_grid(B, 4))) loop_np = 4;
            }
            if (loop_np != 4) {
                plan.split_lds = split_loop_lds_bytes<512>(P.Ks, m);
                plan.split_fn = loop_split_fn<2>(form, P.Ks, g_lu_dbg != nullptr);
                if (fits(d, plan.split_fn, plan.split_nt, plan.split_lds, shared_grid(B, 2))) loop_np = 2;
            }
            if (loop_np > 1) { plan.kind = LOOP_SPLIT; plan.kind_wg = loop_np; }
        }
        // above 512 rows (BASELINE configs[3]: n = 1000): the streaming loop of the symmetric path with TWO workgroups per problem, each
        // streaming one range of whole block columns of H (admm_loop_body_from, NP == 2): twice the registers and LDS under the same
        // matrix (16 % -> 32 % of it on chip), half the stream per CU -- one CU alone pulls 58 GB/s, 29 us per iteration at n = 1000
        if (family_has_form(LOOP_NP2, form) && spd && mode == 2 && P.xchg && P.Ks > SPD_MAXK && P.Ks <= SPD_BIGK && plan.loop_nt == 1024 &&
            k.loop_np2 != 0 && !solo && !(retry & 2)) {
            plan.np2_fn = np2_kernel(form);
            if (fits(d, plan.np2_fn, 1024, plan.loop_lds, shared_grid(B, 2))) { plan.kind = LOOP_NP2; plan.kind_wg = 2; }
        }
        // ... and for batches LARGER than half the CUs (BASELINE configs[4]: 1024 per GPU), where the loop runs one launch per
        // check segment anyway: the same kernel, its pairs taking turns on the chip (FwdParams::split_seg) -- a pair holds its
        // whole matrix in registers for the 15 iterations of a segment where the one-workgroup kernel streams two thirds of it
        // per iteration (B = 1024, n = 500: loop 3.35 -> 8 turns x 4 segments)
        if (spd && mode == 1 && P.xchg && P.Ks >= SPLIT_MINK && P.Ks <= SPD_MAXK && check >= 4 &&
            k.loop_split != 0 && k.loop_split_seg != 0 && !(retry & 2) && !solo && 2 * B > d.cus) {
            plan.split_lds = split_loop_lds_bytes<512>(P.Ks, m);
            plan.split_fn = loop_split_fn<2>(form, P.Ks, false);
            plan.loop_split_seg = fits(d, plan.split_fn, plan.split_nt, plan.split_lds, 0);
        }
    }
    // LU tier, persistent mode, n <= 256, 2 B workgroups resident: the explicit inverse of the KKT matrix in the registers of two
    // workgroups per problem (lqp_dense.hpp) -- float64, many equality rows, non-symmetric Q, control['linsolve'] = 'lu'
    // (the plain form alone, family_has_form: an inverse in registers pays off least where the element-wise step grows)
    if (family_has_form(LOOP_DENSE, form) && !spd && mode == 2 && P.dnx && n <= DENSE_NMAX && k.loop_dense != 0) {
        const int dense_lds = dense_loop_lds_bytes<T>(m);
        if (lu_inverse_lds_bytes<T>(P.Np) <= 160 * 1024 && fits(d, k_admm_loop_dense<T>, DENSE_NT, dense_lds, shared_grid(B, 2))) {
            plan.kind = LOOP_DENSE; plan.kind_lds = dense_lds; plan.kind_wg = 2;
        }
    }
    // ... and for batches that leave most of the chip idle, any n the inverse kernel takes: W workgroups per problem, each with its
    // rows of the inverse in registers (k_admm_loop_dense_w): a matrix-vector product spreads over CUs, triangular solves do not
    if (family_has_form(LOOP_DENSE_W, form) && !spd && mode == 2 && P.dnx && plan.kind != LOOP_DENSE && n > DENSE_NMAX && k.loop_dense_w != 0 && lu_inverse_fits<T>(P.Np) &&
        (size_t)P.dnx_words >= densew_xchg_words<T>(n)) {
        const int densew_lds = densew_lds_bytes<T>(n, m);
        const int tpr = densew_tpr(n, densew_cpt<T>());
        const int W = (n + DENSEW_NT / tpr - 1) / (DENSEW_NT / tpr);
        if (tpr <= 32 && W >= 2 && fits(d, k_admm_loop_dense_w<T>, DENSEW_NT, densew_lds, (long long)W * B)) {
            plan.kind = LOOP_DENSE_W; plan.kind_lds = densew_lds; plan.kind_wg = W; plan.densew_tpr = tpr;
        }
    }
    if constexpr (sizeof(T) == 4) {
        // small problems (n <= 128, e.g. BASELINE configs[1]): 256 threads per QP, the full matrix in registers (k_admm_loop_small)
        if (spd && mode == 2 && plan.kind != LOOP_SPLIT && P.Ks <= 2 && k.loop_small != 0) {
            const int small_lds = small_loop_lds_bytes(m);
            plan.small_fn = small_loop_kernel(form);
            if (fits(d, plan.small_fn, 256, small_lds, B)) { plan.kind = LOOP_SMALL; plan.kind_lds = small_lds; }
        }
        // the equality correction of the first factorisation moves into that kernel (its blocks are in registers there)
        // (ctrl.reserved2 bit 0: the caller will read the corrected H from the workspace afterwards -- lqp_boxqp_unroll_backward --
        //  so the correction must reach global memory: k_spd_end runs)
        // (one launch per check segment, pairs taking turns: the FIRST segment's launch applies it and writes the corrected blocks
        //  back -- from two turns of the chip on; below that k_spd_end on every CU at once is faster: B = 256 1.39 against 1.53 ms
        //  per step, B = 512 2.69 against 2.59)
        const bool seg_eq = plan.loop_split_seg && B >= 2 * d.cus;
        P.eq_in_loop = ((plan.kind == LOOP_SPLIT || seg_eq) && plan.spd_resident && m > 0 && !(ctl->reserved2 & 1) && k.eq_in_loop) ? 1 : 0;
    }
}

// ---- the scheduler ----
template <typename T> void plan_scheduler(FwdParams<T>& P, const lqp_boxqp_ctrl* ctl, const Knobs& k, FwdPlan<T>& plan) {
    const int max_iters = ctl->max_iters, ar_iter = P.ar_iter;
    const bool spd = plan.spd, each = form_each(plan.form);
    // no-host-sync plan (ctrl.reserved == 1, persistent launches): enqueue the WHOLE schedule.
    // Every kernel exits at once when the device-side DONE flag is up, the refactor chains are
    // gated on device, so nothing needs the host; errors are read later by the caller
    // (lqp_boxqp_forward_layout).  Only taken when the number of adaptive-rho events is small.
    // A synchronous call (the default: the reference's semantics) enqueues the same schedule and then waits for the report
    // the last kernel stores into the caller's pinned memory (wait_report) -- not for the stream.
    int n_events = 0;
    for (int a = ar_iter; ctl->adaptive_rho && a < max_iters && a < ctl->adaptive_rho_max_iter; a += ar_iter) ++n_events;
    plan.up_front = (ctl->reserved >= 1 || k.sync_plan != 0) && plan.mode == 2 && n_events <= k.nosync_max_events;
    // (round 6) the two-workgroup loop does not stop at the first iteration at which rho MAY be adapted: it looks at the
    // counters of the check before and only hands over to the continuation kernel when the event changes something
    // (FwdParams::hot_past).  Its range is the whole solve; the continuation launch is enqueued from the first event
    // iteration on and finds its real starting point in status[ST_RESUME].
    // (each: the hot launch ends at the first possible event -- the continuation kernel takes the problem's own decision there)
    plan.hot_past = !each && plan.up_front && plan.kind == LOOP_SPLIT && spd && plan.inkernel_refactor && ctl->adaptive_rho && k.hot_past != 0 &&
                    ar_iter < ctl->adaptive_rho_max_iter && ar_iter < max_iters;
    P.hot_past = plan.hot_past ? 1 : 0;
    // A GIVEN rho is the case in which the adaptation does fire (`rho = 0.01`: three factorisations, 281 iterations,
    // 4.5 ms with everything behind iteration 100 on the continuation kernel).  Enqueue a few rounds of {the event
    // on the gated kernels of the refactorisation, the hot loop again from where it stopped}: each costs a solve that
    // is over ~5 launches that leave at once -- which is why the automatic rho (it practically never adapts) gets none.
    plan.hot_rounds = (ctl->rho_mode != 0 && !each) ? k.hot_rounds : 0;
    // (each: workgroups leave the last launch at different times -- workgroup 0 cannot report the status block from inside it)
    // (L1: the epilogue takes two more outputs, a launch of its own)
    plan.tail_epilogue = k.tail_epilogue != 0 && plan.form == FORM_ALL;
    plan.spec_launches = k.spec_launches;
    plan.factor_launches = spd ? (plan.spd_big_split ? 2 * P.Ks + 2 : plan.spd_split ? (plan.spd_resident ? 3 : P.Ks + 2) : 1) : 2;
    plan.loop_workgroups = plan.loop_split_seg ? 2 : plan.kind_wg;      // (what the loop's launches put on a problem)
}

// Every decision of an attempt and every ensure_lds / occupancy query; launches nothing.  Writes the fields of P that are decisions.
// retry: bit 0 -- the symmetric x-update gave the solve up (not symmetric / not positive definite in f32): pivoted LU;
//        bit 1 -- a pair of the turn-taking two-workgroup loop (split_seg) waited for its partner in vain: the one-workgroup loop
//        bit 2 -- a kernel that shares its problems between workgroups gave up waiting (bounded spins: something else holds the
//                 CUs -- another stream, another process, RCCL): nothing shared this time -- one workgroup per matrix in every
//                 factorisation, host-launched check segments instead of the persistent loop with its grid barrier
template <typename T> int plan_forward(FwdParams<T>& P, const lqp_boxqp_ctrl* ctl, const int retry, const Knobs& k, const Device& d, FwdPlan<T>& plan) {
    const TermArgs term = plan.term;
    plan = FwdPlan<T>(); plan.retry = retry; plan.solo = (retry & 4) != 0; plan.term = term;
    // control['stop'] = 'each': the loop kernels with a per-problem form -- the one-workgroup loop (every size, dtype and m), the small
    // loop and the split loop on two / four workgroups per problem; no other hot kernel, no hot_past, no hot rounds, no 512-thread build
    plan.form = loop_form(P);
    plan.dbg_loop_absent = k.dbg_loop_absent;
    P.xcd_local = k.xcd_local != 0 ? 1 : 0;
    P.dbg_qpass = k.dbg_qpass;      // (bit 0: the second half of the debug buffer; bits 8..: the wave whose stamps the resident sweep records)
    P.dbg = g_lu_dbg; P.dbg_setup = nullptr;
    if (g_lu_dbg && k.dbg_setup) { P.dbg_setup = g_lu_dbg; P.dbg = nullptr; }
    int rc = plan_xupdate(P, ctl, k, d, plan);
    if (!rc) rc = plan_loop_kernels(P, ctl, k, d, plan);
    if (rc) return rc;
    plan_hot_kind(P, ctl, k, d, plan);
    plan_scheduler(P, ctl, k, plan);
    return LQP_OK;
}

// ---- launch steps: they read the plan and decide nothing ----
// factorise (gate == nullptr) or refactorise under the device-side gate of k_rho_update
template <typename T>
int enqueue_factor(hipStream_t st, const FwdParams<T>& P, const FwdPlan<T>& plan, const int* gate, int& n_launch) {
    const int B = P.B;
    if constexpr (sizeof(T) == 4) {
        if (plan.spd) {
            const int lds = spd_factor_lds_bytes(P.m, P.Ks);
            ProfScope ps(st, PC_SPD_INV);
            if (plan.spd_big_split) {
                // 512 < n <= 1024, few problems: two workgroups per matrix, a launch per phase of a pivot step
                hipLaunchKernelGGL(k_spd_begin<>, dim3(shared_grid(B, SPD_NP)), dim3(LQP_NT), lds, st, P, gate);
                if (plan.rho_late_big && gate == nullptr) {
                    hipLaunchKernelGGL(k_spd_rho_big<>, dim3(B), dim3(LQP_NT), 0, st, P);
                    ++n_launch;
                }
                const int f16 = plan.f16;
                for (int k = 0; k < P.Ks; ++k) {
                    const dim3 grd(shared_grid(B, SPD_NP)), blk(LQP_NT);
                    if (plan.fuse2 && k + 1 < P.Ks) {
                        hipLaunchKernelGGL(k_spd_big_step<>, grd, blk, lds, st, P, gate, k, 1 | f16);
                        hipLaunchKernelGGL(k_spd_big_step<>, grd, blk, lds, st, P, gate, k, 4 | f16);
                        hipLaunchKernelGGL(k_spd_big_step<>, grd, blk, lds, st, P, gate, k + 1, 1 | 16 | f16);
                        hipLaunchKernelGGL(k_spd_big_step<>, grd, blk, lds, st, P, gate, k, 8 | f16);
                        ++k;
                        continue;
                    }
                    hipLaunchKernelGGL(k_spd_big_step<>, grd, blk, lds, st, P, gate, k, 1);
                    hipLaunchKernelGGL(k_spd_big_step<>, grd, blk, lds, st, P, gate, k, 2);
                }
                hipLaunchKernelGGL(k_spd_end<>, dim3(B), dim3(LQP_NT), lds, st, P, gate);
                n_launch += 2 * P.Ks + 2;
                return LQP_OK;
            }
            if (plan.spd_split) {
                // few problems: SPD_NP workgroups per matrix, one launch per pivot step (k_spd_begin/step/end)
                if (!(gate == nullptr && P.prep_fused))      // (the first factorisation's blocks: k_spd_prep built them)
                    hipLaunchKernelGGL(k_spd_begin<>, dim3(shared_grid(B, SPD_NP)), dim3(LQP_NT), lds, st, P, gate);
                if (plan.spd_resident) {
                    // all pivot steps in one launch, the matrix in the registers of its two workgroups
                    hipLaunchKernelGGL(plan.rs_fn, dim3((plan.dbg_loop_absent & 2) ? B : shared_grid(B, plan.rs_np)), dim3(RS_NT),
                                       rs_q_lds_bytes(P.Ks), st, P, gate);
                    n_launch += 1;
                } else {
                    for (int k = 0; k < P.Ks; ++k)
                        hipLaunchKernelGGL(k_spd_step<>, dim3(shared_grid(B, SPD_NP)), dim3(LQP_NT), lds, st, P, gate, k, plan.spd_pivot_tasks);
                    n_launch += P.Ks;
                }
                if (!(gate == nullptr && P.eq_in_loop)) hipLaunchKernelGGL(k_spd_end<>, dim3(B), dim3(LQP_NT), lds, st, P, gate);
                n_launch += 2;
                return LQP_OK;
            }
            hipLaunchKernelGGL(P.Ks > SPD_MAXK ? k_spd_inverse<2> : k_spd_inverse<1>, dim3(B), dim3(LQP_NT), lds, st, P, gate);
            ++n_launch;
            return LQP_OK;
        }
    }
    // (scratch of the two-workgroup LU: the head of each problem's packed area -- the pack kernel fills it afterwards)
    const size_t pk_words = packed_blocks(P.K) * LQP_BLK * sizeof(T) / 8;
    int r2 = launch_lu(st, P.M, B, P.N, P.Np, (size_t)P.Np * P.Np, P.piv, P.Np, P.info, gate, nullptr,
                       (unsigned long long*)P.packed, pk_words);
    if (r2) return r2;
    r2 = launch_pack<T>(st, B, P.M, P.N, P.Np, (size_t)P.Np * P.Np, P.piv, P.Np, P.packed, P.dest, gate);
    n_launch += 2;
    return r2;
}

// the epilogue as a launch of its own: the plain one, or the one of the form's term with its two outputs
template <typename T>
void launch_epilogue(hipStream_t st, const FwdParams<T>& P, const FwdPlan<T>& plan) {
    by_form(plan.form, [&](auto f) {
        using TERM = typename decltype(f)::term;
        if constexpr (TERM::kind != 0) hipLaunchKernelGGL((k_fwd_epilogue<T, TERM>), dim3(P.B), dim3(256), 0, st, P, (T*)plan.term.aux, (T*)plan.term.u_box);
        else hipLaunchKernelGGL(k_fwd_epilogue<T>, dim3(P.B), dim3(256), 0, st, P);
    });
}
// everything in front of the loop: the pass over Q (k_spd_prep), setup (its workgroup 0 zeroes status + counter ring), the first
// factorisation, and for the dense tiers X = M^-1
template <typename T>
int enqueue_prologue(hipStream_t st, const FwdParams<T>& P, const FwdPlan<T>& plan, int& n_launch) {
    const int B = P.B;
    if (P.vtrace) HIP_OK(hipMemsetAsync(P.vtrace, 0, sizeof(unsigned int) * 2 * kRing, st));
    if (P.host_report) report_reset(P.host_report, ST_WORDS + 2 * B);      // (before the first launch: see wait_report)
    if constexpr (sizeof(T) == 4) {
        if (P.prep_fused == 1 || P.prep_fused == 2) {
            ProfScope ps(st, PC_SPD_INV);
            hipLaunchKernelGGL(k_spd_prep<>, dim3(shared_grid(B, SPD_NP)), dim3(LQP_NT), spd_prep_lds_bytes(P.Ks), st, P);
            ++n_launch;
        }
    }
    {
        ProfScope ps(st, PC_SETUP);
        hipLaunchKernelGGL(k_fwd_setup<T>, dim3(B), dim3(LQP_NT), setup_lds_bytes<T>(P.n), st, P);
        ++n_launch;
    }
    int rc = enqueue_factor(st, P, plan, nullptr, n_launch);
    if (rc) return rc;
    if (plan.kind == LOOP_DENSE || plan.kind == LOOP_DENSE_W) {
        // X = M^-1 over the LAPACK copy of the factor (the pack kernel has read it; a refactorisation re-assembles M anyway)
        rc = launch_lu_inverse<T>(st, B, P.N, P.packed, packed_blocks(P.K) * LQP_BLK, P.dest, P.Np, P.M, (size_t)P.Np * P.Np, P.Np, nullptr);
        if (rc) return rc;
        ++n_launch;
    }
    by_form(plan.form, [&](auto f) {      // the term's scaled inputs: behind whoever wrote the scaling vector (the setup kernel, or the resident sweep it defers to)
        using TERM = typename decltype(f)::term;
        if constexpr (TERM::kind != 0) {
            ProfScope ps(st, PC_SETUP);
            TermIn<T> in;
            for (int k = 0; k < TERM_IN_MAX; ++k) in.p[k] = (const T*)plan.term.in[k];
            hipLaunchKernelGGL((k_term_setup<T, TERM>), dim3(P.B), dim3(256), 0, st, P, in);
            ++n_launch;
        }
    });
    return LQP_OK;
}

// the first launch of the persistent mode: iterations [0, e), the kernel of plan.kind
template <typename T>
void launch_hot(hipStream_t st, const FwdParams<T>& P, const FwdPlan<T>& plan, const int e, const int ctr_base) {
    const int B = P.B, absent = plan.dbg_loop_absent;
    ProfScope ps(st, PC_LOOP);
    if constexpr (sizeof(T) == 4) switch (plan.kind) {
        case LOOP_SPLIT:
            hipLaunchKernelGGL(plan.split_fn, dim3((absent & 1) ? B : shared_grid(B, plan.kind_wg)), dim3(plan.split_nt), plan.split_lds, st, P, 0, e, ctr_base);
            return;
        case LOOP_SMALL:
            hipLaunchKernelGGL(plan.small_fn, dim3(B), dim3(256), plan.kind_lds, st, P, 0, e, ctr_base);
            return;
        case LOOP_NP2:
            hipLaunchKernelGGL(plan.np2_fn, dim3((absent & 8) ? B : shared_grid(B, 2)), dim3(1024), plan.loop_lds, st, P, 0, e, ctr_base, -1, 1);
            return;
        default: break;
    }
    switch (plan.kind) {
        case LOOP_DENSE:
            hipLaunchKernelGGL(k_admm_loop_dense<T>, dim3(shared_grid(B, 2)), dim3(DENSE_NT), plan.kind_lds, st, P, 0, e, ctr_base);
            return;
        case LOOP_DENSE_W:
            hipLaunchKernelGGL(k_admm_loop_dense_w<T>, dim3(plan.kind_wg * B), dim3(DENSEW_NT), plan.kind_lds, st, P, 0, e, ctr_base, plan.densew_tpr);
            return;
        default:
            hipLaunchKernelGGL(plan.loop_fn, dim3(B), dim3(plan.loop_nt), plan.loop_lds, st, P, 0, e, ctr_base, -1, 1);
    }
}

// an adaptive-rho event on separate kernels: k_rho_update raises the device-side gate, the refactorisation runs under it
template <typename T>
int enqueue_rho_event(hipStream_t st, const FwdParams<T>& P, const FwdPlan<T>& plan, const int slot, const int resume_end, int& n_launch) {
    { ProfScope ps(st, PC_RHO);
      hipLaunchKernelGGL(k_rho_update<T>, dim3(P.B), dim3(LQP_NT), 0, st, P, slot, resume_end); }
    ++n_launch;
    return enqueue_factor(st, P, plan, P.status + ST_GATE, n_launch);
}

// the counter-ring slots of a launch over iterations [it, e): check c counts into slot c % kRing
struct RingSpan {
    long long c_first, c_last;      // first check index >= it, last check index <= e - 1
    int ctr_base, prev_slot;        // slot of c_first; slot of the last check before `it` (-1: none)
    RingSpan(const int it, const int e, const int check)
        : c_first((it + check - 1) / check), c_last((e - 1) / check), ctr_base((int)(c_first % kRing)),
          prev_slot(it > 0 ? ((it - 1) / check) % kRing : -1) {}
};

// what the enqueue knows; the solve's own figures are not on the host yet (-1) -- collect_report / solve_stats fill them in
template <typename T>
void fill_stats(lqp_boxqp_stats* stats, const FwdPlan<T>& plan, const int mode_used, const int n_launch) {
    memset(stats, 0, sizeof(*stats));
    stats->iters = stats->n_factor = stats->n_solve = stats->n_check = -1;
    stats->fail_index = -1; stats->n_launch = n_launch; stats->mode_used = mode_used;
    stats->any_lb = stats->any_ub = -1;
    stats->linsolve_used = plan.spd ? 2 : 1;
    stats->factor_launches = plan.factor_launches;
    stats->loop_workgroups = plan.loop_workgroups;
    stats->loop_kind = plan.loop_split_seg ? (int)LOOP_SPLIT : (mode_used == 1 ? (int)LOOP_ONE : (int)plan.kind);
}

// why an attempt gave up, for forward_impl's retry loop
enum GaveUp {
    GU_NONE = 0,
    GU_NOT_SPD,             // Qs + rho I not positive definite in f32 (first factorisation or an adaptive-rho one; on some rank)
    GU_LU_TIMEOUT,          // a shared LU never met its partner
    GU_SEG_TIMEOUT,         // a pair of the turn-taking loop (split_seg) waited for its partner in vain
    GU_SHARED_TIMEOUT       // another shared sweep / loop / grid barrier gave up
};
struct Attempt {
    int status; GaveUp why;
    Attempt(int s) : status(s), why(GU_NONE) {}
    Attempt(GaveUp w) : status(LQP_OK), why(w) {}
};

// ---- the whole schedule up front (plan.up_front) ----
template <typename T>
Attempt run_planned(hipStream_t st, const FwdParams<T>& P, const FwdPlan<T>& plan, const lqp_boxqp_ctrl* ctl, lqp_boxqp_stats* stats,
                    int n_launch) {
    const int B = P.B, check = P.check_solved, max_iters = ctl->max_iters, ar_iter = P.ar_iter;
    const bool spd = plan.spd;
    int rc = LQP_OK;
    int it = 0;
    bool epilogue_done = false;
    bool resume_next = false;       // the next continuation launch starts where the hot kernel says it stopped
    while (it < max_iters) {
        // the adaptive-rho step of iteration `it` runs as the prologue of the continuation kernel
        bool event = ctl->adaptive_rho && it > 0 && it % ar_iter == 0 && it < ctl->adaptive_rho_max_iter;
        if (event && !plan.inkernel_refactor) {      // f64 / symmetric path: separate gated kernels
            rc = enqueue_rho_event(st, P, plan, ((it - 1) / check) % kRing, 0, n_launch);
            if (rc) return rc;
            event = false;
        }
        int e = max_iters;
        const bool hot_past = it == 0 && plan.hot_past;
        if (ctl->adaptive_rho && !((spd || plan.inkernel_refactor) && it > 0) && !hot_past) {      // (the continuation kernel walks through its events itself)
            const int a = (it / ar_iter + 1) * ar_iter;
            if (a < ctl->adaptive_rho_max_iter) e = std::min(e, a);
        }
        // a launch may hold at most kRing/2 checks (counter ring); longer tails are split
        e = std::min(e, it + (kRing / 2) * check);
        const RingSpan s(it, e, check);
        if (s.c_last >= kRing) {      // these slots were used one ring ago: clear exactly them (stream-ordered)
            for (long long c = std::max<long long>(s.c_first, kRing); c <= s.c_last; ) {
                const int s0 = (int)(c % kRing);
                const long long run = std::min<long long>(s.c_last - c + 1, kRing - s0);
                HIP_OK(hipMemsetAsync(P.counters + (size_t)s0 * CT_WORDS, 0,
                                      sizeof(unsigned int) * CT_WORDS * (size_t)run, st));
                c += run;
            }
        }
        bool last_tail = false;
        if (it == 0) {
            launch_hot(st, P, plan, e, s.ctr_base);
            resume_next = hot_past;
            if (hot_past) {
                // rounds of {the event on the gated kernels of the refactorisation, the hot loop again from where it stopped}
                for (int rd = 0; rd < plan.hot_rounds; ++rd) {
                    rc = enqueue_rho_event(st, P, plan, -1, max_iters, n_launch);
                    if (rc) return rc;
                    if constexpr (sizeof(T) == 4) {
                        FwdParams<float> Pr = P;
                        Pr.hot_resume = 1;
                        Pr.eq_in_loop = 0;          // (k_spd_end has corrected the new blocks in global memory)
                        ProfScope ps(st, PC_LOOP);
                        hipLaunchKernelGGL(plan.split_fn, dim3(shared_grid(B, plan.kind_wg)), dim3(plan.split_nt), plan.split_lds, st, Pr,
                                           ar_iter, e, RingSpan(ar_iter, e, check).ctr_base);
                        ++n_launch;
                    }
                }
                e = ar_iter;          // (the continuation launch below is enqueued for [first event, ...): see plan.hot_past)
            }
        } else {
            // the last continuation launch ends with the epilogue (one launch and its boundary less)
            last_tail = e >= max_iters && plan.tail_epilogue;
            ProfScope ps(st, PC_LOOP_TAIL);
            hipLaunchKernelGGL(plan.tail_fn, dim3(B), dim3(LQP_NT), plan.tail_lds, st,
                               P, it, e, s.ctr_base, s.prev_slot,
                               ((event || spd || plan.inkernel_refactor) ? 3 : 1) | (last_tail ? 4 : 0) | (resume_next ? 8 : 0));
            resume_next = false;
        }
        ++n_launch;
        it = e;
        epilogue_done = last_tail;
    }
    if (!epilogue_done) {
        ProfScope ps(st, PC_EPILOGUE);
        launch_epilogue(st, P, plan);
        ++n_launch;
    }
    if (hipGetLastError() != hipSuccess) return LQP_ERR_HIP;
    // reserved == 1: nothing is waited for.  reserved == 2 with a host report, the split call: everything is enqueued; the caller
    // does its own host work (output views, bookkeeping) while the GPU runs and then collects the report with lqp_boxqp_forward_finish
    if (ctl->reserved == 1 || (ctl->reserved == 2 && P.host_report)) {
        if (stats) fill_stats(stats, plan, ctl->reserved == 1 ? 3 : 4, n_launch);
        return LQP_OK;
    }
    // ---- synchronous call: status block, info and flag words of every problem ----
    std::vector<int> rep_copy;
    const int* rep = P.host_report;
    if (!rep) {                     // (a C caller without pinned memory: three small copies and a stream wait)
        rep_copy.resize(ST_WORDS + 2 * B);
        HIP_OK(hipMemcpyAsync(rep_copy.data(), P.status, sizeof(int) * ST_WORDS, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(rep_copy.data() + ST_WORDS, P.info, sizeof(int) * B, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(rep_copy.data() + ST_WORDS + B, P.bflags, sizeof(int) * B, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        rep = rep_copy.data();
    }
    lqp_boxqp_stats local;
    lqp_boxqp_stats* so = stats ? stats : &local;
    fill_stats(so, plan, 2, n_launch);
    rc = collect_report(st, rep, rep == P.host_report, B, max_iters, check, so);
    if (rc == LQP_ERR_TIMEOUT && !spd && !t_single_wg_lu && !(flags_timeout_loop(rep))) return GU_LU_TIMEOUT;
    if (rc == LQP_ERR_TIMEOUT && !plan.solo) return GU_SHARED_TIMEOUT;
    if (rc == LQP_RETRY_LU) return GU_NOT_SPD;
    return rc;
}

// ---- host-driven chunks: check segments (mode 1) or persistent launches (mode 2), the status read back after each chunk ----
template <typename T>
Attempt run_chunked(hipStream_t st, const FwdParams<T>& P, const FwdPlan<T>& plan, const lqp_boxqp_ctrl* ctl, lqp_boxqp_stats* stats,
                    int n_launch) {
    const int B = P.B, check = P.check_solved, max_iters = ctl->max_iters, ar_iter = P.ar_iter, mode = plan.mode;
    const bool spd = plan.spd;
    int rc = LQP_OK;
    int h_status[ST_WORDS];
    memset(h_status, 0, sizeof(h_status));
    int it = 0;
    long long zeroed_upto = kRing;     // check indices [0, zeroed_upto) have clean slots
    bool done = false, singular_checked = false;
    int nfactor_seen = 0;
    int chunk_cap = plan.spec_launches;
    int fail_index = -1;
    while (it < max_iters && !done) {
        int in_chunk = 0;
        const int cap_now = (mode == 2) ? 1 : chunk_cap;       // persistent: the kernel itself stops at convergence
        while (it < max_iters && in_chunk < cap_now) {
            // adaptive-rho event at the start of iteration `it` (:237)
            const bool tail_events = spd && mode == 2;       // symmetric path, persistent: events inside the tail kernel
            if (!tail_events && ctl->adaptive_rho && it > 0 && it % ar_iter == 0 && it < ctl->adaptive_rho_max_iter) {
                rc = enqueue_rho_event(st, P, plan, ((it - 1) / check) % kRing, 0, n_launch);
                if (rc) return rc;
            }
            // end of this launch
            int e = max_iters;
            const int next_check = ((it + check - 1) / check) * check;
            if (mode == 1) e = std::min(e, next_check + 1);
            else e = std::min(e, next_check + 1 + (kMaxChecksPerLaunch - 1) * check);
            if (ctl->adaptive_rho && !(tail_events && it > 0)) {
                const int a = (it / ar_iter + 1) * ar_iter;
                if (a < ctl->adaptive_rho_max_iter) e = std::min(e, a);
            }
            if (e <= it) e = it + 1;
            const RingSpan s(it, e, check);
            while (s.c_last >= zeroed_upto) {
                const int s0 = (int)(zeroed_upto % kRing);
                HIP_OK(hipMemsetAsync(P.counters + (size_t)s0 * CT_WORDS, 0, sizeof(unsigned int) * CT_WORDS * (kRing / 2), st));
                zeroed_upto += kRing / 2;
            }
            { const bool first = (mode == 2 && it == 0) || mode == 1;
              if (first && mode == 2) {
                  launch_hot(st, P, plan, e, s.ctr_base);
              } else if (plan.loop_split_seg) {
                  if constexpr (sizeof(T) == 4) {
                      FwdParams<float> Ps = P;
                      Ps.split_seg = 1;
                      Ps.seg_prev_slot = s.prev_slot;
                      if (it > 0) Ps.eq_in_loop = 0;
                      ProfScope ps(st, PC_LOOP);
                      hipLaunchKernelGGL(plan.split_fn, dim3(shared_grid(B, 2)), dim3(plan.split_nt), plan.split_lds, st, Ps, it, e, s.ctr_base);
                  }
              } else {
                  ProfScope ps(st, first ? PC_LOOP : PC_LOOP_TAIL);
                  hipLaunchKernelGGL(first ? plan.loop_fn : plan.tail_fn, dim3(B), dim3(first ? plan.loop_nt : LQP_NT),
                                     first ? plan.loop_lds : plan.tail_lds, st, P, it, e,
                                     s.ctr_base, s.prev_slot, mode == 2 ? ((tail_events && !first) ? 3 : 1) : 0);
              } }
            ++n_launch;
            ++in_chunk;
            it = e;
            if (ctl->check_hook && mode == 1 && ((e - 1) % check) == 0) {
                // strict global stop: all-reduce this check's counters over the ranks before anything reads them
                const long long c_idx = (e - 1) / check;
                if (ctl->check_hook(ctl->check_hook_user, (void*)st, (void*)(P.counters + (size_t)(c_idx % kRing) * CT_WORDS),
                                    (int)c_idx) != 0)
                    return LQP_ERR_HIP;
            }
        }
        // ---- close the chunk: did the last check stop the loop? ----
        if (it > 0 && ((it - 1) % check) == 0) {
            // did the last check of this chunk stop the loop?  (tiny kernel, own name in traces)
            const int prev_slot = ((it - 1) / check) % kRing;
            ProfScope ps(st, PC_MISC);
            hipLaunchKernelGGL(k_check_done<>, dim3(1), dim3(64), 0, st, P.status, P.counters, prev_slot, it - 1);
            ++n_launch;
        }
        // the epilogue only reads state: run it now so that the common case (converged in this chunk)
        // pays no host round trip between the loop and its outputs; a later chunk simply re-runs it
        { ProfScope ps(st, PC_EPILOGUE);
          launch_epilogue(st, P, plan); }
        ++n_launch;
        // (with a host report the epilogue has left status and info words in pinned host memory: one wait, no copies)
        if (!P.host_report) HIP_OK(hipMemcpyAsync(h_status, P.status, sizeof(h_status), hipMemcpyDeviceToHost, st));
        auto fetch_status = [&]() -> int {
            HIP_OK(hipStreamSynchronize(st));
            if (P.host_report)
                for (int i = 0; i < ST_WORDS; ++i) h_status[i] = ((const volatile int*)P.host_report)[i];
            return LQP_OK;
        };
        // A failed factorisation ends or restarts the solve.  With a check hook (strict global stop over batch shards)
        // that decision must be the same on every rank -- a rank that restarted alone would pair its collectives with
        // other checks of its peers -- so the local verdict goes through the hook (SUM over the ranks) first.
        auto after_factorisation = [&]() -> Attempt {
            int rcf = first_failure(st, P.info, B, &fail_index, P.host_report ? P.host_report + ST_WORDS : nullptr);      // synchronises
            if (rcf == LQP_OK || rcf == LQP_ERR_SINGULAR) { const int r4 = fetch_status(); if (r4) return r4; }
            if (rcf == LQP_ERR_TIMEOUT && !spd && !t_single_wg_lu) return GU_LU_TIMEOUT;
            if (rcf != LQP_OK && rcf != LQP_ERR_SINGULAR) return rcf;
            bool leave_spd = rcf == LQP_ERR_SINGULAR && spd, singular = rcf == LQP_ERR_SINGULAR && !spd;
            if (ctl->check_hook) {
                int vote[CT_WORDS] = {leave_spd ? 1 : 0, singular ? 1 : 0, 0, 0};
                HIP_OK(hipMemcpyAsync(P.status + ST_VOTE, vote, sizeof(vote), hipMemcpyHostToDevice, st));
                if (ctl->check_hook(ctl->check_hook_user, (void*)st, (void*)(P.status + ST_VOTE), -1) != 0) return LQP_ERR_HIP;
                HIP_OK(hipMemcpyAsync(vote, P.status + ST_VOTE, sizeof(vote), hipMemcpyDeviceToHost, st));
                HIP_OK(hipStreamSynchronize(st));
                leave_spd = vote[0] > 0;
                singular = vote[1] > 0;
            }
            if (singular) {                                           // (fail_index -1: the singular problem is on another rank)
                if (stats) { memset(stats, 0, sizeof(*stats)); stats->fail_index = fail_index; }
                return LQP_ERR_SINGULAR;
            }
            if (leave_spd) return GU_NOT_SPD;
            return LQP_OK;
        };
        if (singular_checked) { const int r4 = fetch_status(); if (r4) return r4; }
        if (!singular_checked || h_status[ST_NFACTOR] != nfactor_seen) {      // the first factorisation, or an adaptive-rho one ran in this chunk
            singular_checked = true;
            const Attempt a = after_factorisation();
            if (a.why != GU_NONE || a.status) return a;
        }
        nfactor_seen = h_status[ST_NFACTOR];
        if (h_status[ST_TIMEOUT]) {
            // The pairs of the turn-taking loop become resident together only while the dispatcher hands workgroups out in
            // blockIdx order onto an otherwise idle chip; when something else holds CUs (another stream, RCCL kernels) a pair can
            // wait for a partner that is not resident.  Its spin is bounded (0.5 s), the kernels drain, and the solve is run again
            // from its setup on the loop that needs nobody (degrade, do not fail).
            if (plan.loop_split_seg && !(plan.retry & 2)) return GU_SEG_TIMEOUT;
            if (!plan.solo) return GU_SHARED_TIMEOUT;      // (the same for every other shared schedule)
            return LQP_ERR_TIMEOUT;
        }
        done = h_status[ST_DONE] != 0;
        chunk_cap = std::min(chunk_cap * 2, 64);
    }
    if (hipGetLastError() != hipSuccess) return LQP_ERR_HIP;
    if (form_term(plan.form)) {
        // a weight that is negative or not finite (k_term_setup marks the problem's flag word; the epilogue has reported it)
        std::vector<int> fl(B);
        if (P.host_report) for (int i = 0; i < B; ++i) fl[i] = ((const volatile int*)P.host_report)[ST_WORDS + B + i];
        else { HIP_OK(hipMemcpyAsync(fl.data(), P.bflags, sizeof(int) * B, hipMemcpyDeviceToHost, st)); HIP_OK(hipStreamSynchronize(st)); }
        for (int i = 0; i < B; ++i)
            if (fl[i] & kTermFlag[form_term(plan.form)]) {
                if (stats) { memset(stats, 0, sizeof(*stats)); stats->fail_index = i; }
                return LQP_ERR_INVALID;
            }
    }
    if (stats) {
        fill_stats(stats, plan, mode, n_launch);
        solve_stats(stats, h_status, max_iters, check);
    }
    return LQP_OK;
}

// sets t_single_wg_lu from enter() to the end of the scope, unless an enclosing scope has set it already
struct SoloScope {
    bool on = false;
    void enter() { if (!t_single_wg_lu) { on = true; t_single_wg_lu = true; } }
    ~SoloScope() { if (on) t_single_wg_lu = false; }
};

// carve, then plan / run / decide until an attempt ends the solve.  A remedy is taken at most once: the run functions name a cause
// only while its remedy is untried (retry bit clear, t_single_wg_lu clear) and in the order LU before bit 2, bit 1 before bit 2;
// after that the failure is the status (a singular problem, a time-out with nothing shared left to give up)
template <typename T>
int forward_impl(hipStream_t st, int B, int n, int m, const void* Q, const void* p, const void* A, const void* b,
                 const void* lb, const void* ub, const lqp_boxqp_ctrl* ctl, const void* rho_in, void* x, void* z,
                 void* u, void* lams, void* nus, void* rho_out, lqp_boxqp_stats* stats, void* ws, size_t ws_bytes,
                 int retry = 0, const double eps_prim_inf = 0.0, const double eps_dual_inf = 0.0, const TermArgs* term = nullptr) {
    // (eps_prim_inf > 0: lqp_boxqp_forward_detect; either > 0: lqp_boxqp_forward_certify; term: lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber)
    FwdLayout<T> L = carve_forward<T>(ws, B, n, m);
    const LoopForm asked = loop_form(term ? term->kind : 0, (ctl->reserved2 & 8) != 0, eps_prim_inf > 0.0 || eps_dual_inf > 0.0, eps_dual_inf > 0.0);
    if (ws_bytes < L.bytes_for(asked)) return LQP_ERR_WORKSPACE;
    {
        FwdParams<T>& P = L.P;
        if (term) { P.term = term->kind; P.termv = (T*)L.term_area; }
        P.Q = (const T*)Q; P.p = (const T*)p; P.A = (const T*)A; P.b = (const T*)b;
        P.lb = (const T*)lb; P.ub = (const T*)ub; P.rho_in = (const T*)rho_in; P.beta_in = (const T*)ctl->beta_in;
        P.x = (T*)x; P.z = (T*)z; P.u = (T*)u; P.lams = (T*)lams; P.nus = (T*)nus; P.rho_out = (T*)rho_out;
        P.scale = ctl->scale; P.bound_flags_in = (const int*)ctl->bound_flags_in;
        // verbose: the largest primal / dual error of the batch at every check (lqp_boxqp_check_trace)
        if (ctl->reserved2 & 4) P.vtrace = L.vtrace_area;
        // per-problem stopping (control['stop'] = 'each'); a strict global stop over shards is its opposite
        if (ctl->reserved2 & 8) {
            if (ctl->check_hook) return LQP_ERR_INVALID;
            P.pstat = L.pstat_area;
            if (form_snapshots(asked)) {
                P.snap = (T*)L.snap_area; P.snap_stride = snap_stride(n, m, asked == FORM_CERTIFY);
                P.eps_pinf = (T)eps_prim_inf; P.eps_dinf = (T)eps_dual_inf;
            }
        }
        each_ws_note(ws, P.pstat != nullptr);
        P.host_report = (int*)ctl->host_report;
        P.zero_words = (int)(((char*)(P.counters + (size_t)kRing * CT_WORDS) - (char*)P.status) / sizeof(int));
        P.rho_mode = ctl->rho_mode; P.beta_mode = ctl->beta_mode;
        P.check_solved = ctl->check_solved < 1 ? 1 : ctl->check_solved;
        P.adaptive_rho = ctl->adaptive_rho;
        P.eps_abs = (T)ctl->eps_abs; P.eps_rel = (T)ctl->eps_rel; P.rho_value = (T)ctl->rho_value;
        P.rho_min = (T)ctl->rho_min; P.rho_max = (T)ctl->rho_max;
        P.ar_tol = (T)ctl->adaptive_rho_tol; P.ar_inv_tol = (T)(1.0 / ctl->adaptive_rho_tol);
        P.ar_thr = (T)ctl->adaptive_rho_threshold; P.beta_value = (T)ctl->beta_value;
        P.ar_iter = ctl->adaptive_rho_iter < 1 ? 1 : ctl->adaptive_rho_iter;
        P.ar_max = ctl->adaptive_rho_max_iter; P.ring = kRing;
        const double alpha = ctl->alpha == 0.0 ? 1.0 : ctl->alpha;       // (0: not set)
        P.alpha = (T)alpha; P.alpha_c = (T)(1.0 - alpha); P.relax = alpha != 1.0 ? 1 : 0;
    }
    Device d;
    if (!current_device_cus(&d.dev, &d.cus)) return LQP_ERR_HIP;
    SoloScope one_wg_lu;
    for (;;) {
        const Knobs k = knobs();            // one snapshot of the switches per attempt (a copy: LQP_ENV_NOCACHE re-reads in place)
        if (retry & 4) one_wg_lu.enter();
        FwdParams<T> P = L.P;
        FwdPlan<T> plan;
        if (term) plan.term = *term;
        int rc = plan_forward(P, ctl, retry, k, d, plan);
        if (rc) return rc;
        int n_launch = 0;
        if (form_snapshots(plan.form)) { hipLaunchKernelGGL(k_snap_init<T>, dim3((2 * B + 255) / 256), dim3(256), 0, st, P.snap, P.snap_stride, B); ++n_launch; }
        rc = enqueue_prologue(st, P, plan, n_launch);
        if (rc) return rc;
        const Attempt a = plan.up_front ? run_planned(st, P, plan, ctl, stats, n_launch) : run_chunked(st, P, plan, ctl, stats, n_launch);
        switch (a.why) {
        case GU_NONE: return a.status;
        case GU_NOT_SPD: retry |= 1; break;             // the LU path takes the solve
        case GU_LU_TIMEOUT: one_wg_lu.enter(); break;   // once more, one workgroup per matrix
        case GU_SEG_TIMEOUT: retry |= 2; break;         // the one-workgroup loop
        case GU_SHARED_TIMEOUT: retry |= 4; break;      // once more with nothing shared
        }
    }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// lu_only: the arrays of one pivoted-LU solve and nothing else (lqp_kkt_solve)
template <typename T>
size_t carve_backward(void* ws, int B, int n, int m, BwdParams<T>& P, const bool lu_only = false) {
    P.B = B; P.n = n; P.m = m; P.N = n + m;
    P.Np = round_up(P.N, LQP_NB); P.K = P.Np / LQP_NB;
    Carver c(ws);
    P.info = c.take<int>(B);
    P.piv = c.take<int>((size_t)B * P.Np);
    P.dest = c.take<int>((size_t)B * P.Np);
    P.rhs = c.take<T>((size_t)B * P.Np);
    if (!lu_only) {
        P.rhs2 = c.take<T>((size_t)B * P.Np);
        P.bsc = c.take<T>((size_t)B * P.Np);
        P.fidx = c.take<int>((size_t)B * n);
        P.nred = c.take<int>(B);
    }
    P.M = c.take<T>((size_t)B * P.Np * P.Np);
    P.packed = c.take<T>((size_t)B * packed_blocks(P.K) * LQP_BLK);
    return c.off + kAlign;
}

// dynamic LDS of the backward's kernels (k_bwd_chol_solve: bwd_chol_lds_bytes, lqp_boxqp.hpp)
inline int bwd_build_chol_lds_bytes(int n, int) { return (2 * round_up(n, 8) + LQP_NW + 8 + round_up(n, 64) + 64) * 4; }      // fl | wtot | the KKT form's diagonal weights | the equilibration
inline int bwd_build_reduced_lds_bytes(int n, int) { return (round_up(n, 8) + LQP_NW + 8) * 4; }                               // fl | wtot
template <typename T> inline int bwd_residual_lds_bytes(int n, int m) { return (round_up(n, 8) + round_up(m > 0 ? m : 1, 8)) * (int)sizeof(T) + round_up(n, 8) * 4; }      // dvf | dn | fl
template <typename T> inline int bwd_epilogue_lds_bytes(int n, int m) { return (2 * n + m + 8) * (int)sizeof(T); }

// one backward call as its entry point received it (lqp_boxqp_backward_fp, _fp_prefactor, _backward_kkt)
struct BwdCall {
    hipStream_t st = nullptr;
    int dtype = LQP_F32, B = 0, n = 0, m = 0;
    const void *g = nullptr, *x = nullptr, *u = nullptr, *lams = nullptr, *nus = nullptr, *Q = nullptr, *A = nullptr, *lb = nullptr,
               *ub = nullptr, *rho_in = nullptr;
    const void* curv = nullptr;         // lqp_boxqp_backward_fp_curv: BwdParams::curv, or null
    int rho_mode = 1; double rho_value = 1.0;
    void *dQ = nullptr, *dp = nullptr, *dA = nullptr, *db = nullptr, *dlb = nullptr, *dub = nullptr;
    int32_t* fail_index = nullptr;      // null: the call neither waits nor repeats anything
    void *ws = nullptr, *host_report = nullptr; size_t ws_bytes = 0;
    int linsolve = 1;                   // 1 | 2, with LQP_BWD_PREFACTORED / LQP_BWD_REPORTED
    bool kkt = false, prefactor = false;      // the KKT-system backward (BwdParams::kkt) | the call ahead of the cotangent: phase 1
};

// BF_CHOL: blocked Cholesky of Q_FF (the fixed-point and the KKT backward alike, P.kkt tells the kernels); the pivoted LU of
// BF_LU_REDUCED: the bordered free-set system, BF_LU_FULL: the reference's full system (LQP_BWD_FULL), BF_LU_KKT: the reduced KKT system
enum BwdForm { BF_CHOL, BF_LU_REDUCED, BF_LU_FULL, BF_LU_KKT };
typedef void (*BwdCholFn)(const BwdParams<float>);
template <typename T> struct BwdPlan {
    BwdParams<T> P;                     // what every kernel of the attempt receives
    BwdForm form = BF_LU_REDUCED;
    int phase = 0;                      // 0: one call, 1: up to the factor (no cotangent needed), 2: from the cotangent on (= P.phase)
    const int* nvec = nullptr;          // the reduced system's sizes for the LU chain (null: N rows each)
    bool reset_report = false;          // the report words are this call's: -1 into each before the first launch
    bool polls = false;                 // a caller that waits polls the report words; else first_failure waits for the stream
    bool report_info = false;           // k_report_info right behind the LU
    bool refine = false;                // one refinement step of the LU form
    BwdCholFn chol_fn = nullptr;
    int build_lds = 0, chol_lds = 0, residual_lds = 0, epilogue_lds = 0;
    dim3 build_grid, residual_grid, epilogue_grid;
};

// Every decision of one attempt, from one snapshot of the switches; launches nothing.  retry (backward_impl): bit 0 = the LU form,
// bit 1 = one workgroup per matrix -- either way one call in full, whatever phases the caller asked for.
template <typename T>
int plan_backward(const BwdCall& c, const Knobs& k, const int retry, BwdPlan<T>& plan) {
    BwdParams<T>& P = plan.P;
    const int B = c.B, n = c.n, m = c.m;
    const int flags = retry ? 0 : c.linsolve & (LQP_BWD_PREFACTORED | LQP_BWD_REPORTED);
    const int linsolve = retry ? 1 : c.linsolve & ~(LQP_BWD_PREFACTORED | LQP_BWD_REPORTED);
    // ---- form.  Default: solve on the free set only (see k_bwd_build_reduced); LQP_BWD_FULL=1 keeps the full system.
    // linsolve 2: the caller vouches for a symmetric Q (the forward's symmetric x-update checked it): the reduced system goes
    // through a blocked Cholesky of Q_FF instead of the pivoted LU of the bordered matrix -- in float32; float64 takes the LU form
    P.kkt = c.kkt ? 1 : 0;
    P.reduced = (k.bwd_full && !c.kkt) ? 0 : 1;
    const int Kmax = round_up(n, LQP_NB) / LQP_NB;
    const int nr = m >= 3 ? 4 : 2;                   // (four right-hand sides per round of the block solves)
    const bool chol = sizeof(T) == 4 && P.reduced && linsolve == 2 && k.bwd_chol && Kmax <= SPD_BIGK && m <= SPD_MAXM &&
                      bwd_chol_lds_bytes(n, m, nr) <= 160 * 1024;
    plan.form = chol ? BF_CHOL : !P.reduced ? BF_LU_FULL : c.kkt ? BF_LU_KKT : BF_LU_REDUCED;
    P.chol = chol ? 1 : 0;
    plan.nvec = P.reduced ? P.nred : nullptr;
    // ---- phase.  The Cholesky and the reduced LU form come in two calls too (ABI 11): 1 = free set, system, factor (packed) -- none
    // of them needs the cotangent --, 2 = gather the cotangent over the free set, solve (+ refinement), epilogue.  The
    // full-system form and the KKT backward are one call: nothing is enqueued for their prefactor call
    int phase = retry ? 0 : c.prefactor ? 1 : ((flags & LQP_BWD_PREFACTORED) && !c.kkt) ? 2 : 0;
    if (plan.form == BF_LU_FULL || plan.form == BF_LU_KKT) {
        if (phase == 1) return LQP_ERR_UNSUPPORTED;
        phase = 0;
    }
    plan.phase = P.phase = phase;
    // ---- report words.  A solve-only call whose prefactor call has reported into them neither resets nor stores them again
    // (with LQP_BWD_EARLY=0 the epilogue reports: the words are this call's to reset and to wait for)
    P.host_report = (int*)c.host_report;
    P.early_report = k.bwd_early != 0 ? 1 : 0;
    P.reported = ((flags & LQP_BWD_REPORTED) && phase == 2 && P.host_report && P.early_report) ? 1 : 0;
    plan.reset_report = P.host_report && !P.reported;
    plan.polls = P.host_report && k.sync_plan != 0;
    // a caller that waits (or a prefactor call: its report buffer is the backward call's): the LU is the step that can fail or
    // time out -- its info words right behind it, see k_report_info
    plan.report_info = !chol && phase != 2 && P.host_report && (phase == 1 || (P.early_report && c.fail_index));
    P.lu_reported = (!chol && (plan.report_info || P.reported)) ? 1 : 0;
    // ---- build (enqueue_build: system and right-hand side, in phase 2 the right-hand side alone), factor, solve
    if (!k.bwd_equil) P.bsc = nullptr;
    plan.build_lds = chol ? bwd_build_chol_lds_bytes(n, m) : (P.reduced && phase != 2) ? bwd_build_reduced_lds_bytes(n, m) : 0;
    // (k_bwd_build_chol's split has never consulted LQP_SPLIT2; k_bwd_gather_rhs and k_bwd_build take one workgroup per problem)
    plan.build_grid = chol ? dim3(B, small_batch_split(B)) : (P.reduced && phase != 2) ? dim3(B, small_batch_split(B, k.split2 != 0)) : dim3(B);
    if (chol) {
        if constexpr (sizeof(T) == 4) {
            plan.chol_fn = nr == 4 ? k_bwd_chol_solve<4> : k_bwd_chol_solve<0>;
#if LQP_PIV_MFMA
            // (not the KKT backward: its weights span 1e-8 .. 1e8, and dlb / dub = lam dx / slack divide the dx of a variable at its
            //  bound by 1e-8: with the two-half products they came out at 5 to 19 times the error of a float32 LAPACK solve, with
            //  float32 products at 1.2 times at most -- tests/kkt_table.py, row chol_bwdf16off_n330)
            if (k.spd_f16 != 0 && k.bwd_f16 != 0 && !c.kkt) plan.chol_fn = nr == 4 ? k_bwd_chol_solve<4, true> : k_bwd_chol_solve<0, true>;
#endif
        }
        plan.chol_lds = bwd_chol_lds_bytes(n, m, nr);
        P.la_maxk = !k.bwd_lookahead ? 0 : (Kmax < SPD_MAXK ? Kmax : SPD_MAXK - 1);
        P.piv_cols = k.piv_cols != 0 ? 1 : 0;
        const int rc = ensure_lds((const void*)plan.chol_fn, plan.chol_lds);
        if (rc) return rc;
    }
    // one refinement step: residual with the original entries (double accumulation), correction solve
    plan.refine = plan.form == BF_LU_REDUCED && k.bwd_refine && phase != 1;
    P.refine = plan.refine ? 1 : 0;
    plan.residual_lds = bwd_residual_lds_bytes<T>(n, m);
    plan.residual_grid = dim3(B, small_batch_split(B, k.split2 != 0));
    // ---- epilogue: row slabs per problem, fill the chip when the batch is small
    if (phase != 1) {
        plan.epilogue_lds = bwd_epilogue_lds_bytes<T>(n, m);
        plan.epilogue_grid = dim3(B, k.epi_slabs < 0 ? small_batch_split(B) : k.epi_slabs);
        const int rc = ensure_lds((const void*)k_bwd_epilogue<T>, plan.epilogue_lds);
        if (rc) return rc;
    }
    return LQP_OK;
}

// ---- the launch steps: they read the plan and decide nothing ----
template <typename T>
void enqueue_build(hipStream_t st, const BwdPlan<T>& plan) {
    const BwdParams<T>& P = plan.P;
    if (plan.form == BF_CHOL && plan.phase == 2) return;      // (k_bwd_chol_solve gathers the cotangent itself)
    ProfScope ps(st, PC_BWD_BUILD);
    if (plan.form == BF_CHOL) {
        if constexpr (sizeof(T) == 4) hipLaunchKernelGGL(k_bwd_build_chol<>, plan.build_grid, dim3(LQP_NT), plan.build_lds, st, P);
    } else if (plan.phase == 2) hipLaunchKernelGGL(k_bwd_gather_rhs<T>, plan.build_grid, dim3(256), 0, st, P);
    else if (P.reduced) hipLaunchKernelGGL(k_bwd_build_reduced<T>, plan.build_grid, dim3(LQP_NT), plan.build_lds, st, P);
    else hipLaunchKernelGGL(k_bwd_build<T>, plan.build_grid, dim3(LQP_NT), 0, st, P);
}

// (the Cholesky kernels exist in float32 only: plan_backward never names this form for float64)
template <typename T>
void enqueue_chol(hipStream_t st, const BwdPlan<T>& plan) {
    if constexpr (sizeof(T) == 4) {
        ProfScope ps(st, PC_BWD_CHOL);
        hipLaunchKernelGGL(plan.chol_fn, dim3(plan.P.B), dim3(LQP_NT), plan.chol_lds, st, plan.P);
    }
}

// The pivoted-LU chain on the system carve_backward laid out, for the backward's LU forms and lqp_kkt_solve: factor (the packed
// factor's buffer is the shared LUs' scratch until the pack fills it), [the info words into the report buffer], pack, solve.
// Phase 1 stops behind the pack, phase 2 is the solve alone.
template <typename T>
int enqueue_lu_chain(hipStream_t st, const BwdParams<T>& P, const int* nvec, const int phase, const bool report_info) {
    const size_t mstride = (size_t)P.Np * P.Np;
    if (phase != 2) {
        int rc = launch_lu(st, P.M, P.B, P.N, P.Np, mstride, P.piv, P.Np, P.info, nullptr, nvec, (unsigned long long*)P.packed,
                           packed_blocks(P.K) * LQP_BLK * sizeof(T) / 8);
        if (rc) return rc;
        if (report_info) {
            ProfScope ps(st, PC_MISC);
            hipLaunchKernelGGL(k_report_info<>, dim3((P.B + 255) / 256), dim3(256), 0, st, (const int*)P.info, P.host_report, P.B);
        }
        rc = launch_pack<T>(st, P.B, P.M, P.N, P.Np, mstride, P.piv, P.Np, P.packed, P.dest, nullptr, nvec);
        if (rc || phase == 1) return rc;
    }
    return launch_solve<T>(st, P.B, P.packed, P.N, P.dest, P.rhs, 1, (size_t)P.Np, 1, 0, nvec);
}

template <typename T>
int enqueue_refinement(hipStream_t st, const BwdPlan<T>& plan) {
    const BwdParams<T>& P = plan.P;
    { ProfScope ps(st, PC_BWD_BUILD);
      hipLaunchKernelGGL(k_bwd_residual<T>, plan.residual_grid, dim3(LQP_NT), plan.residual_lds, st, P); }
    return launch_solve<T>(st, P.B, P.packed, P.N, P.dest, P.rhs2, 1, (size_t)P.Np, 1, 0, plan.nvec);
}

template <typename T>
void enqueue_epilogue(hipStream_t st, const BwdPlan<T>& plan) {
    ProfScope ps(st, PC_BWD_EPILOGUE);
    hipLaunchKernelGGL(k_bwd_epilogue<T>, plan.epilogue_grid, dim3(LQP_NT), plan.epilogue_lds, st, plan.P);
}

// why an attempt gave up, for backward_impl's retry loop
// (BG_CHOL_NOT_SPD: Q_FF not positive definite in f32; BG_LU_TIMEOUT: a shared LU never met its partner, info word -7)
enum BwdGaveUp { BG_NONE = 0, BG_CHOL_NOT_SPD, BG_LU_TIMEOUT };
struct BwdOutcome { int status, fail_index; BwdGaveUp why; };

// The info words of a finished attempt as (status, first failing problem, cause).  torch.linalg.solve checks info (and waits)
// too.  A cause is named only while its remedy is untried: the Cholesky form is planned on the first attempt only, and
// t_single_wg_lu says that the shared LUs are off already.
template <typename T>
BwdOutcome read_outcome(hipStream_t st, const BwdPlan<T>& plan) {
    const BwdParams<T>& P = plan.P;
    BwdOutcome o = {LQP_OK, -1, BG_NONE};
    if (plan.polls) {                   // (backward_impl has waited for the words)
        bool gave_up = false;
        for (int i = 0; i < P.B; ++i) {
            const int v = ((const volatile int*)P.host_report)[i];
            if (v != 0 && o.fail_index < 0) o.fail_index = i;
            gave_up = gave_up || v == -7;
        }
        o.status = gave_up ? LQP_ERR_TIMEOUT : o.fail_index >= 0 ? LQP_ERR_SINGULAR : LQP_OK;
    } else
        o.status = first_failure(st, P.info, P.B, &o.fail_index, P.host_report);
    if (o.status == LQP_ERR_TIMEOUT && plan.form != BF_CHOL && !t_single_wg_lu) o.why = BG_LU_TIMEOUT;
    else if (o.status == LQP_ERR_SINGULAR && plan.form == BF_CHOL) o.why = BG_CHOL_NOT_SPD;
    return o;
}

// carve, then plan / enqueue / read / decide until an attempt ends the call.  Each remedy is taken at most once (read_outcome);
// a time-out is looked at first, and the two causes exclude each other (one needs an LU form, the other the Cholesky form)
template <typename T>
int backward_impl(const BwdCall& c) {
    const hipStream_t st = c.st;
    BwdParams<T> P0;
    memset(&P0, 0, sizeof(P0));
    if (c.ws_bytes < carve_backward<T>(c.ws, c.B, c.n, c.m, P0)) return LQP_ERR_WORKSPACE;
    P0.g = (const T*)c.g; P0.x = (const T*)c.x; P0.u = (const T*)c.u; P0.lams = (const T*)c.lams; P0.nus = (const T*)c.nus;
    P0.Q = (const T*)c.Q; P0.A = (const T*)c.A; P0.lb = (const T*)c.lb; P0.ub = (const T*)c.ub; P0.rho_in = (const T*)c.rho_in;
    P0.rho_value = (T)c.rho_value; P0.rho_mode = c.rho_mode; P0.curv = (const T*)c.curv;
    P0.dQ = (T*)c.dQ; P0.dp = (T*)c.dp; P0.dA = (T*)c.dA; P0.db = (T*)c.db; P0.dlb = (T*)c.dlb; P0.dub = (T*)c.dub;
    P0.dbg = g_lu_dbg;
    SoloScope one_wg_lu;
    for (int retry = 0;;) {
        const Knobs k = knobs();            // one snapshot of the switches per attempt (a copy: LQP_ENV_NOCACHE re-reads in place)
        if (retry & 2) one_wg_lu.enter();
        BwdPlan<T> plan;
        plan.P = P0;
        int rc = plan_backward(c, k, retry, plan);
        if (rc) return rc;
        if (plan.reset_report) report_reset(plan.P.host_report, c.B);
        enqueue_build(st, plan);
        if (plan.form == BF_CHOL) enqueue_chol(st, plan);
        else rc = enqueue_lu_chain(st, plan.P, plan.nvec, plan.phase, plan.report_info);
        if (rc) return rc;
        if (plan.phase == 1) return last_error();          // (the factor is in the workspace; nothing to wait for)
        if (plan.refine) rc = enqueue_refinement(st, plan);
        if (rc) return rc;
        enqueue_epilogue(st, plan);
        if (last_error()) return LQP_ERR_HIP;
        if (!c.fail_index) return LQP_OK;
        // The kernel that reports stores the info words into the caller's pinned memory as it STARTS: the call returns while the
        // gradients are still being written (stream-ordered results)
        if (plan.polls) {
            rc = wait_report(st, plan.P.host_report, c.B);
            if (rc) return rc;
        }
        const BwdOutcome o = read_outcome(st, plan);
        switch (o.why) {
        case BG_NONE: *c.fail_index = o.fail_index; return o.status;
        case BG_LU_TIMEOUT: retry |= 2; break;             // once more, one workgroup per matrix
        case BG_CHOL_NOT_SPD: retry |= 1; break;           // once more on the LU form
        }
    }
}
inline int backward_call(const BwdCall& c) { return c.dtype == LQP_F32 ? backward_impl<float>(c) : backward_impl<double>(c); }

// ---------------------------------------------------------------------------
// LU / solve / KKT entry points
// ---------------------------------------------------------------------------
inline size_t lu_scratch_u64(int N) { return N > 512 ? (luw_scratch_words<double>(N) + 1) / 2 : (size_t)LU2_SCR_WORDS; }
template <typename T>
size_t carve_lu(void* ws, int B, int N, T*& M, int*& piv, unsigned long long*& scr) {
    const int Np = round_up(N, LQP_NB);
    Carver c(ws);
    piv = c.take<int>((size_t)B * Np);
    M = c.take<T>((size_t)B * Np * Np);
    scr = c.take<unsigned long long>((size_t)B * lu_scratch_u64(N));      // (hand-off words of the two-workgroup LU / messages of the wide one)
    return c.off + kAlign;
}

template <typename T>
int lu_factor_impl(hipStream_t st, int B, int N, void* Mio, int32_t* piv_out, int32_t* info_out, void* ws, size_t ws_bytes) {
    T* M; int* piv; unsigned long long* scr;
    const size_t need = carve_lu<T>(ws, B, N, M, piv, scr);
    if (ws_bytes < need) return LQP_ERR_WORKSPACE;
    const int Np = round_up(N, LQP_NB);
    hipLaunchKernelGGL(k_copy_matrix<T>, dim3(B), dim3(LQP_NT), 0, st, (const T*)Mio, N, (size_t)N * N, M, Np, (size_t)Np * Np, N);
    int rc = launch_lu(st, M, B, N, Np, (size_t)Np * Np, piv, Np, info_out, nullptr, nullptr, scr, lu_scratch_u64(N));
    if (rc) return rc;
    hipLaunchKernelGGL(k_copy_matrix<T>, dim3(B), dim3(LQP_NT), 0, st, (const T*)M, Np, (size_t)Np * Np, (T*)Mio, N, (size_t)N * N, N);
    hipLaunchKernelGGL(k_copy_ints<int>, dim3(B), dim3(256), 0, st, (const int*)piv, Np, (int*)piv_out, N, N);
    return last_error();
}

template <typename T> size_t packed_bytes_t(int B, int N) {
    const int K = round_up(N, LQP_NB) / LQP_NB;
    Carver c(nullptr);
    c.take<int>((size_t)B * K * LQP_NB);
    c.take<T>((size_t)B * packed_blocks(K) * LQP_BLK);
    return c.off + kAlign;
}
template <typename T> void carve_packed(void* buf, int B, int N, int*& dest, T*& packed) {
    const int K = round_up(N, LQP_NB) / LQP_NB;
    Carver c(buf);
    dest = c.take<int>((size_t)B * K * LQP_NB);
    packed = c.take<T>((size_t)B * packed_blocks(K) * LQP_BLK);
}

template <typename T>
int lu_pack_impl(hipStream_t st, int B, int N, const void* LU, const int32_t* piv, void* buf) {
    int* dest; T* packed;
    carve_packed<T>(buf, B, N, dest, packed);
    return launch_pack<T>(st, B, (const T*)LU, N, N, (size_t)N * N, (const int*)piv, N, packed, dest, nullptr);
}
template <typename T>
int lu_solve_packed_impl(hipStream_t st, int B, int N, int k, const void* buf, void* rhs) {
    int* dest; T* packed;
    carve_packed<T>((void*)buf, B, N, dest, packed);
    return launch_solve<T>(st, B, packed, N, dest, (T*)rhs, k, (size_t)N * k, k, 1);
}

template <typename T>
int kkt_solve_impl(hipStream_t st, int B, int n, int m, const void* Q, const void* p, const void* A, const void* b,
                   void* x, void* nus, int32_t* fail_index, void* ws, size_t ws_bytes) {
    BwdParams<T> P;
    memset(&P, 0, sizeof(P));
    if (ws_bytes < carve_backward<T>(ws, B, n, m, P, true)) return LQP_ERR_WORKSPACE;
    hipLaunchKernelGGL(k_kkt_build<T>, dim3(B), dim3(LQP_NT), 0, st, (const T*)Q, (const T*)p, (const T*)A, (const T*)b,
                       n, m, P.Np, P.M, P.rhs, P.info);
    int rc = enqueue_lu_chain(st, P, nullptr, 0, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_kkt_unpack<T>, dim3(B), dim3(256), 0, st, (const T*)P.rhs, n, m, P.Np, (T*)x, (T*)nus);
    if (last_error()) return LQP_ERR_HIP;
    if (fail_index) {
        int fi = -1;
        rc = first_failure(st, P.info, B, &fi);
        *fail_index = fi;
        if (rc) return rc;
    }
    return LQP_OK;
}

// ---------------------------------------------------------------------------
// unroll=True: backward through the unrolled loop (lqp_unroll.hpp)
// ---------------------------------------------------------------------------
// one unroll call as its entry point received it (lqp_boxqp_unroll_backward, _backward_lu, _tape_segment, _tape_finish)
struct UnrollCall {
    hipStream_t st = nullptr;
    int dtype = LQP_F32, B = 0, n = 0, m = 0, iters = 0;
    const void* fwd_ws = nullptr; size_t fwd_ws_bytes = 0;      // the solve's own workspace (null: _tape_finish reads none)
    void* scratch = nullptr; size_t scratch_bytes = 0;
    const void* g = nullptr;
    void *dQs = nullptr, *dps = nullptr, *dAs = nullptr, *dbs = nullptr, *dlbs = nullptr, *dubs = nullptr, *drho = nullptr, *dD = nullptr;
    // _tape_segment alone: x-updates [k0, k1) with the epoch's packed factor and rho (lqp_unroll.hpp, UnrollLuParams)
    int k0 = 0, k1 = 0, mode = 0, inj_k = -1;
    const void *packed_buf = nullptr, *rho = nullptr, *inj = nullptr;
    void* state = nullptr;
    void **zrows = nullptr, **urows = nullptr, **xrows = nullptr;
};

// UP: UnrollParams, the tape of the symmetric x-update (float32), or UnrollLuParams<T>, the tape of the pivoted LU (any m)
template <typename UP> constexpr bool kSymTape = std::is_same<UP, UnrollParams>::value;
// the scratch of a tape of TT x-updates, U zeroed and carved -> bytes
template <typename T, typename UP>
size_t carve_tape(void* ws, int B, int n, int m, int TT, bool segments, UP& U) {
    memset(&U, 0, sizeof(U));
    Carver cv(ws);
    const size_t rows = (size_t)B * TT, mm = m > 0 ? m : 1;
    U.X = cv.take<T>(rows * n);
    U.W = cv.take<T>(rows * n);
    U.DX = cv.take<T>(rows * n);
    U.NU = cv.take<T>(rows * mm);
    if constexpr (!kSymTape<UP>) U.DNU = cv.take<T>(rows * mm);
    U.MK = cv.take<signed char>(rows * n);
    if constexpr (!kSymTape<UP>) {
        if (segments) {             // (a tape in segments also keeps z_{k+1}, u_{k+1}: the rho adaptation reads them)
            U.Zr = cv.take<T>(rows * n);
            U.Ur = cv.take<T>(rows * n);
        }
        U.inj_k = -1;
    }
    return cv.off + kAlign;
}

// Both workspaces of a call, checked in one order by every entry: the forward's (P: null when the entry reads none), what the symmetric
// x-update takes, the tape's scratch.  U comes back carved and otherwise zero.
template <typename T, typename UP>
int carve_unroll_call(const UnrollCall& c, const bool segments, FwdParams<T>* P, UP& U, int& TT) {
    if (P) {
        const FwdLayout<T> L = carve_forward<T>((void*)c.fwd_ws, c.B, c.n, c.m);
        if (c.fwd_ws_bytes < L.bytes) return LQP_ERR_WORKSPACE;
        *P = L.P;
        if (kSymTape<UP> && (P->Ks > SPD_BIGK || c.m > SPD_MAXM)) return LQP_ERR_UNSUPPORTED;      // (what the symmetric x-update takes)
    }
    TT = c.iters + 1;
    return c.scratch_bytes < carve_tape<T>(c.scratch, c.B, c.n, c.m, TT, segments, U) ? LQP_ERR_WORKSPACE : LQP_OK;
}
template <typename T, typename UP> void tape_outputs(const UnrollCall& c, UP& U) {
    U.g = (const T*)c.g;
    U.dps = (T*)c.dps; U.dlbs = (T*)c.dlbs; U.dubs = (T*)c.dubs; U.dD = (T*)c.dD; U.dAs = (T*)c.dAs; U.dbs = (T*)c.dbs; U.drho = (T*)c.drho;
}

// ---- the symmetric tape (float32): which sweep a call launches, decided before the launch ----
typedef void (*UnrollOneFn)(const FwdParams<float>, const UnrollParams);
typedef void (*UnrollSplitFn)(const FwdParams<float>, const UnrollParams, const unsigned int);
struct UnrollSymPlan {
    UnrollSplitFn split_fn = nullptr;       // k_unroll_sweep_split: two workgroups per QP, or ...
    UnrollOneFn one_fn = nullptr;           // ... k_unroll_sweep: one
    int lds = 0, grid = 0;
};
// Ks (5 ... SPD_MAXK) -> the instance of the two-workgroup sweep and its LDS bytes (m <= 1 has an instance of its own at Ks = 8 only)
UnrollSplitFn unroll_split_fn(const int Ks, const int m, int& lds) {
#define LQP_KS_CASE(KS) case KS: lds = unroll_split_lds_bytes<KS>(m); return k_unroll_sweep_split<KS, SPD_MAXM>
    switch (Ks) {
        case 8: lds = unroll_split_lds_bytes<8>(m); return m <= 1 ? k_unroll_sweep_split<8, 1> : k_unroll_sweep_split<8, SPD_MAXM>;
        LQP_KS_CASE(7); LQP_KS_CASE(6); default: LQP_KS_CASE(5);
    }
#undef LQP_KS_CASE
}
// two workgroups per QP when half the chip would idle (the split loop's products, lqp_unroll.hpp: k_unroll_sweep_split) and all of
// them are resident at once; launches nothing
UnrollSymPlan plan_unroll_sym(const FwdParams<float>& P, const int rl, const Knobs& k) {
    UnrollSymPlan plan;
    Device d;
    if (P.xchg && P.Ks >= 5 && P.Ks <= SPD_MAXK && k.unroll_split != 0) {
        const UnrollSplitFn fn = unroll_split_fn(P.Ks, P.m, plan.lds);
        if (current_device_cus(&d.dev, &d.cus) && fits(d, fn, 512, plan.lds, shared_grid(P.B, 2))) plan.split_fn = fn;
    }
    if (plan.split_fn) {
        plan.grid = (k.dbg_loop_absent & 4) ? P.B : shared_grid(P.B, 2);
    } else {
        plan.one_fn = P.m <= 1 ? k_unroll_sweep<1> : k_unroll_sweep<SPD_MAXM>;
        plan.lds = unroll_lds_bytes(P.m, P.Ks, rl);
        plan.grid = P.B;
    }
    return plan;
}

int unroll_backward_sym_impl(const UnrollCall& c) {
    FwdParams<float> P; UnrollParams U; int T;
    int rc = carve_unroll_call<float>(c, false, &P, U, T);
    if (rc) return rc;
    U.T = T;
    U.rl = unroll_lds_blocks(c.m, P.Ks);
    tape_outputs<float>(c, U);
    const UnrollSymPlan plan = plan_unroll_sym(P, U.rl, knobs());
    if (plan.split_fn) {
        ProfScope ps(c.st, PC_UNROLL);
        hipLaunchKernelGGL(plan.split_fn, dim3(plan.grid), dim3(512), plan.lds, c.st, P, U, g_unroll_run.fetch_add(1u));
    } else {
        rc = ensure_lds((const void*)plan.one_fn, plan.lds);
        if (rc) return rc;
        ProfScope ps(c.st, PC_UNROLL);
        hipLaunchKernelGGL(plan.one_fn, dim3(plan.grid), dim3(LQP_NT), plan.lds, c.st, P, U);
    }
    if (c.dQs) {
        ProfScope ps(c.st, PC_UNROLL);
        const int tiles = (c.n + 63) / 64;
        hipLaunchKernelGGL(k_unroll_outer<>, dim3(tiles, tiles, c.B), dim3(256), 0, c.st, (const float*)U.DX, (const float*)U.X,
                           (float*)c.dQs, c.n, T);
    }
    return last_error();
}

// ---- the tape whose x-update is the pivoted LU (float32 / float64, any m): the launch steps ----
template <typename T>
int enqueue_lu_sweep(hipStream_t st, const FwdParams<T>& P, const UnrollLuParams<T>& U) {
    const int lds = unroll_lu_lds_bytes<T>(P.Np);
    auto fn = k_unroll_sweep_lu<T>;
    const int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    ProfScope ps(st, PC_UNROLL);
    hipLaunchKernelGGL(fn, dim3(P.B), dim3(LQP_NT), lds, st, P, U);
    return LQP_OK;
}
// what is summed over the whole tape once it has been walked: Asbar / bsbar from the scratch rows, Qsbar
template <typename T>
void enqueue_tape_sums(hipStream_t st, const UnrollLuParams<T>& U, int B, int n, int m, void* dQs) {
    if (m > 0) {
        ProfScope ps(st, PC_UNROLL);
        int slabs = (m * n + 255) / 256;
        if (slabs > 64) slabs = 64;
        hipLaunchKernelGGL(k_unroll_lu_eq<T>, dim3(B, slabs), dim3(256), 0, st, U, n, m);
    }
    if (dQs) {
        ProfScope ps(st, PC_UNROLL);
        const int tiles = (n + 63) / 64;
        hipLaunchKernelGGL(k_unroll_outer_any<T>, dim3(tiles, tiles, B), dim3(256), 0, st, (const T*)U.DX, (const T*)U.X, (T*)dQs, n, U.T_);
    }
}

template <typename T>
int unroll_backward_lu_impl(const UnrollCall& c) {
    FwdParams<T> P; UnrollLuParams<T> U; int TT;
    int rc = carve_unroll_call<T>(c, false, &P, U, TT);
    if (rc) return rc;
    U.T_ = TT;
    tape_outputs<T>(c, U);
    rc = enqueue_lu_sweep<T>(c.st, P, U);
    if (rc) return rc;
    enqueue_tape_sums<T>(c.st, U, c.B, c.n, c.m, c.dQs);
    return last_error();
}

// one segment [k0, k1) of a tape whose factor changes along it (a solve in which rho was adapted): replay and / or reverse walk
// with the epoch's packed factor and rho (lqp_unroll.hpp, UnrollLuParams)
template <typename T>
int unroll_tape_segment_impl(const UnrollCall& c) {
    FwdParams<T> P; UnrollLuParams<T> U; int TT;
    const int rc = carve_unroll_call<T>(c, true, &P, U, TT);
    if (rc) return rc;
    if (c.zrows) *c.zrows = U.Zr;
    if (c.urows) *c.urows = U.Ur;
    if (c.xrows) *c.xrows = U.X;
    if (c.k1 <= c.k0) return LQP_OK;             // (a query of the row pointers)
    U.T_ = TT; U.k0 = c.k0; U.k1 = c.k1; U.mode = c.mode;
    if (c.packed_buf) {
        int* dest; T* packed;
        carve_packed<T>((void*)c.packed_buf, c.B, P.N, dest, packed);
        U.packed_ov = packed; U.dest_ov = dest;
    }
    U.rho_ov = (const T*)c.rho;
    U.state = (T*)c.state;
    U.inj_k = c.inj ? c.inj_k : -1; U.inj = (const T*)c.inj;
    tape_outputs<T>(c, U);
    const int rs = enqueue_lu_sweep<T>(c.st, P, U);
    return rs ? rs : last_error();
}

// ... and what is summed over the whole tape once every segment has been walked
template <typename T>
int unroll_tape_finish_impl(const UnrollCall& c) {
    UnrollLuParams<T> U; int TT;
    const int rc = carve_unroll_call<T>(c, true, (FwdParams<T>*)nullptr, U, TT);
    if (rc) return rc;
    U.T_ = TT; U.dAs = (T*)c.dAs; U.dbs = (T*)c.dbs;
    enqueue_tape_sums<T>(c.st, U, c.B, c.n, c.m, c.dQs);
    return last_error();
}

// one call for either dtype: f is a generic lambda over a value of the element type, by_dtype(dtype, [&](auto t) { ... decltype(t) ... })
template <typename F> inline auto by_dtype(const int dtype, F f) { return dtype == LQP_F32 ? f(float()) : f(double()); }

bool bad_dims(int dtype, int B, int n, int m) {
    return (dtype != LQP_F32 && dtype != LQP_F64) || B < 1 || n < 1 || m < 0;
}

}  // namespace

// ---- the element-wise kernels around lqp_boxqp_backward_fp (log: lqp_boxqp_backward_fp_curv) in the backwards of those solves
//      (csrc/lqp_boxqp.hpp): dtype, dims and the pointers that must be there; one thread per element of [B][n] ----
inline bool elementwise_ok(int dtype, int B, int n, std::initializer_list<const void*> required) {
    bool ok = (dtype == LQP_F32 || dtype == LQP_F64) && B >= 1 && n >= 1;
    for (const void* q : required) ok = ok && q != nullptr;
    return ok;
}
template <typename F> int elementwise(void* stream, int dtype, int B, int n, F launch) {
    const size_t total = (size_t)B * n;
    by_dtype(dtype, [&](auto t) { launch(t, dim3((unsigned int)((total + 255) / 256)), (hipStream_t)stream, total); return 0; });
    return last_error();
}

extern "C" {

int lqp_abi_version(void) { return LQP_ABI_VERSION; }
size_t lqp_boxqp_ctrl_bytes(void) { return sizeof(lqp_boxqp_ctrl); }

void lqp_profile_enable(int on) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    g_prof_on = on != 0;
}

void lqp_profile_reset(void) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    for (auto& r : g_prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    g_prof_recs.clear();
    for (int i = 0; i < PC_COUNT; ++i) { g_prof_ms[i] = 0.0; g_prof_n[i] = 0; }
}

void lqp_debug_set_lu_counters(void* device_buf) { g_lu_dbg = (unsigned long long*)device_buf; }

// test aid: occupy `blocks` workgroups of 512 threads (one CU each when LDS-bound kernels run next to it) for `usec`
// microseconds on `stream` -- the co-residency tests run the two-workgroup schedules beside it
__global__ __launch_bounds__(512) void k_debug_spin(const unsigned long long ticks) {
    extern __shared__ __attribute__((aligned(32))) char smem[];
    smem[threadIdx.x] = 0;                  // (touch the LDS so that the allocation is real)
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
int lqp_debug_spin(void* stream, int blocks, int usec, int lds_bytes) {
    if (blocks < 1 || usec < 0 || usec > 2000000 || lds_bytes < 512) return LQP_ERR_INVALID;
    const int rc = ensure_lds((const void*)k_debug_spin, lds_bytes);
    if (rc) return rc;
    hipLaunchKernelGGL(k_debug_spin, dim3(blocks), dim3(512), lds_bytes, (hipStream_t)stream, (unsigned long long)usec * 100ull);
    return last_error();
}

// test aid: the XCD every workgroup of a `blocks`-workgroup launch lands on (what the XCD-aware exchange asks at run time)
__global__ __launch_bounds__(512) void k_debug_xcd(int* __restrict__ out) {
    if (threadIdx.x == 0) out[blockIdx.x] = (int)my_xcd();
}
int lqp_debug_xcd(void* stream, int blocks, void* out_dev) {
    if (blocks < 1 || !out_dev) return LQP_ERR_INVALID;
    hipLaunchKernelGGL(k_debug_xcd, dim3(blocks), dim3(512), 0, (hipStream_t)stream, (int*)out_dev);
    return last_error();
}

int lqp_debug_lu_inverse(void* stream, int dtype, int B, int N, const void* packed_buf, void* X_out) {
    if (bad_dims(dtype, B, N, 0) || !packed_buf || !X_out || N > (dtype == LQP_F32 ? 2048 : 1024)) return LQP_ERR_INVALID;
    const int K = round_up(N, LQP_NB) / LQP_NB;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        int* dest; T* packed;
        carve_packed<T>((void*)packed_buf, B, N, dest, packed);
        return launch_lu_inverse<T>((hipStream_t)stream, B, N, packed, packed_blocks(K) * LQP_BLK, dest, K * LQP_NB, (T*)X_out,
                                    (size_t)N * N, N, nullptr);
    });
}

int lqp_debug_chol_solve(void* stream, int B, int Kmax, const void* packed, const void* kb, int nrhs, int nr, int which,
                         const void* V, void* X_out) {
    if (B < 1 || Kmax < 1 || Kmax > SPD_MAXK || nrhs < 1 || nrhs > 32 || (nr != 2 && nr != 4) || (which != 0 && which != 1) ||
        !packed || !kb || !V || !X_out) return LQP_ERR_INVALID;
    const int lds = debug_chol_solve_lds_bytes(Kmax, nrhs, nr);
    auto fn = nr == 4 ? k_debug_chol_solve<4> : k_debug_chol_solve<2>;
    const int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(fn, dim3(B), dim3(LQP_NT), lds, (hipStream_t)stream, (const float*)packed, (const int*)kb, (const float*)V,
                       (float*)X_out, Kmax, nrhs, which);
    return last_error();
}

int lqp_debug_chol_factor(void* stream, int B, int Kmax, void* packed_inout, const void* nf, int f16, int which, void* info_out) {
    if (B < 1 || Kmax < 1 || Kmax > SPD_MAXK || (f16 != 0 && f16 != 1) || (which != 0 && which != 1) || !packed_inout || !nf || !info_out)
        return LQP_ERR_INVALID;
#if !LQP_PIV_MFMA
    if (f16) return LQP_ERR_UNSUPPORTED;
#endif
    // LDS and look-ahead limit as plan_backward sets them for n = 64 Kmax
    const int a0 = spd_lds_bytes(Kmax);
    const int lds = (Kmax < SPD_MAXK && chol_la_lds_bytes(Kmax) > a0) ? chol_la_lds_bytes(Kmax) : a0;
    const int la_maxk = !knobs().bwd_lookahead ? 0 : (Kmax < SPD_MAXK ? Kmax : SPD_MAXK - 1);
    auto fn = f16 ? k_debug_chol_factor<true> : k_debug_chol_factor<false>;
    const int rc = ensure_lds((const void*)fn, lds);
    if (rc) return rc;
    if (hipMemsetAsync(info_out, 0, (size_t)B * sizeof(int), (hipStream_t)stream) != hipSuccess) return LQP_ERR_HIP;
    hipLaunchKernelGGL(fn, dim3(B), dim3(LQP_NT), lds, (hipStream_t)stream, (float*)packed_inout, (const int*)nf, (int*)info_out, Kmax,
                       la_maxk, which);
    return last_error();
}

int lqp_profile_classes(void) { return PC_COUNT; }

const char* lqp_profile_class_name(int c) {
    static const char* names[PC_COUNT] = {"fwd_setup", "lu_factor", "pack", "admm_loop", "rho_update", "fwd_epilogue",
                                          "bwd_build", "packed_solve", "bwd_epilogue", "misc", "admm_loop_tail",
                                          "spd_inverse", "eq_correct", "bwd_cholesky", "unroll_backward", "unroll_scaling"};
    return (c >= 0 && c < PC_COUNT) ? names[c] : "?";
}

int lqp_profile_get(double* total_ms, long long* launches, int n) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    for (auto& r : g_prof_recs) {
        if (hipEventSynchronize(r.b) != hipSuccess) return LQP_ERR_HIP;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return LQP_ERR_HIP;
        g_prof_ms[r.cls] += ms;
        g_prof_n[r.cls] += 1;
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    g_prof_recs.clear();
    for (int i = 0; i < n && i < PC_COUNT; ++i) { total_ms[i] = g_prof_ms[i]; launches[i] = g_prof_n[i]; }
    return LQP_OK;
}

const char* lqp_status_string(int s) {
    switch (s) {
        case LQP_OK: return "ok";
        case LQP_ERR_INVALID: return "invalid argument";
        case LQP_ERR_WORKSPACE: return "workspace too small";
        case LQP_ERR_SINGULAR: return "singular matrix (exactly zero pivot)";
        case LQP_ERR_HIP: return "HIP runtime error";
        case LQP_ERR_TIMEOUT: return "in-kernel grid barrier timed out";
        case LQP_ERR_UNSUPPORTED: return "size not supported by this build (n + m <= 4096 in float32, 2048 in float64)";
        case LQP_ERR_NOT_SPD: return "matrix outside the symmetric x-update: repeat with linsolve = 1";
        default: return "unknown status";
    }
}

int lqp_boxqp_forward_layout(int dtype, int B, int n, int m, size_t* status_offset, size_t* status_bytes,
                             size_t* info_offset, size_t* info_bytes) {
    if (bad_dims(dtype, B, n, m) || !status_offset || !status_bytes || !info_offset || !info_bytes) return LQP_ERR_INVALID;
    char* base = (char*)4096;       // any non-null base: only offsets are used
    by_dtype(dtype, [&](auto t) {
        const FwdLayout<decltype(t)> L = carve_forward<decltype(t)>(base, B, n, m);
        *status_offset = (char*)L.P.status - base; *info_offset = (char*)L.P.info - base;
    });
    *status_bytes = sizeof(int) * ST_WORDS;
    *info_bytes = sizeof(int) * (size_t)B;
    return LQP_OK;
}

size_t lqp_boxqp_forward_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes; });
}

size_t lqp_boxqp_forward_detect_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes_for(FORM_DETECT); });
}

// lqp_boxqp_forward (both thresholds 0: no detection), lqp_boxqp_forward_detect (eps_dual_inf = 0) and lqp_boxqp_forward_certify
static int forward_entry(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                         const void* b, const void* lb, const void* ub, const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                         void* x, void* z, void* u, void* lams, void* nus, void* rho_out, lqp_boxqp_stats* stats,
                         void* workspace, size_t workspace_bytes, const double eps_prim_inf, const double eps_dual_inf,
                         const TermArgs* term = nullptr) {
    if (bad_dims(dtype, B, n, m) || !Q || !p || !lb || !ub || !ctrl || !x || !z || !u || !lams || !rho_out || !workspace)
        return LQP_ERR_INVALID;
    if (m > 0 && (!A || !b || !nus)) return LQP_ERR_INVALID;
    if (ctrl->rho_mode == 2 && !rho_in) return LQP_ERR_INVALID;
    if (ctrl->beta_mode == 2 && !ctrl->beta_in) return LQP_ERR_INVALID;
    if (ctrl->max_iters < 1) return LQP_ERR_INVALID;
    // over-relaxation: 0 = not set = 1; else inside (0, 2) (NaN fails both comparisons), and the factor kept for the unroll sweep
    // (reserved2 bit 0) belongs to the plain step its tapes replay
    if (ctrl->alpha != 0.0 && !(ctrl->alpha > 0.0 && ctrl->alpha < 2.0)) return LQP_ERR_INVALID;
    if (ctrl->alpha != 0.0 && ctrl->alpha != 1.0 && (ctrl->reserved2 & 1)) return LQP_ERR_INVALID;
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int retry0 = (ctrl->reserved2 & 2) ? 4 : 0;      // (bit 1: the caller has seen a shared schedule time out -- nothing shared)
    return by_dtype(dtype, [&](auto t) {
        return forward_impl<decltype(t)>(st, B, n, m, Q, p, A, b, lb, ub, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace, workspace_bytes, retry0, eps_prim_inf, eps_dual_inf, term);
    });
}

int lqp_boxqp_forward(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                      const void* b, const void* lb, const void* ub, const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                      void* x, void* z, void* u, void* lams, void* nus, void* rho_out, lqp_boxqp_stats* stats,
                      void* workspace, size_t workspace_bytes) {
    return forward_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace,
                         workspace_bytes, 0.0, 0.0);
}

int lqp_boxqp_forward_detect(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                             const void* b, const void* lb, const void* ub, const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                             void* x, void* z, void* u, void* lams, void* nus, void* rho_out, lqp_boxqp_stats* stats,
                             void* workspace, size_t workspace_bytes, double eps_prim_inf) {
    // refused before anything is touched: a threshold outside (0, 1) (NaN fails both comparisons), no per-problem stop, a check
    // hook (a global stop), the factor kept for the unroll sweep
    if (!(eps_prim_inf > 0.0 && eps_prim_inf < 1.0)) return LQP_ERR_INVALID;
    if (!ctrl || !(ctrl->reserved2 & 8) || (ctrl->reserved2 & 1) || ctrl->check_hook) return LQP_ERR_INVALID;
    return forward_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace,
                         workspace_bytes, eps_prim_inf, 0.0);
}

// ---- the solves with a separable term: lqp_boxqp_forward_l1 / _soft / _log / _pwl / _huber ----
size_t lqp_boxqp_forward_l1_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes_for(FORM_L1); });
}
size_t lqp_boxqp_forward_soft_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes_for(FORM_SOFT); });
}
size_t lqp_boxqp_forward_log_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes_for(FORM_LOG); });
}
size_t lqp_boxqp_forward_pwl_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes_for(FORM_PWL); });
}
size_t lqp_boxqp_forward_huber_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes_for(FORM_HUBER); });
}

// Refused before anything is touched: a null pointer of the term's own, the per-problem stop (no instance of its kernels with a term), a
// check hook, the factor kept for the unroll sweep (its tape replays the plain step), and the rho = 0 one-shot -- a solve with a term
// always iterates, whatever the bounds: all of them infinite is an ordinary case here
static int term_entry(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                      const void* b, const void* lb, const void* ub, const TermArgs& term, const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                      void* x, void* z, void* u, void* lams, void* nus, void* rho_out, lqp_boxqp_stats* stats,
                      void* workspace, size_t workspace_bytes) {
    for (int k = 0; k < kTermInputs[term.kind]; ++k) if (!term.in[k]) return LQP_ERR_INVALID;
    if (!term.aux || !term.u_box) return LQP_ERR_INVALID;
    if (!ctrl || (ctrl->reserved2 & (8 | 1)) || ctrl->check_hook) return LQP_ERR_INVALID;
    if (ctrl->rho_mode == 1 && !(ctrl->rho_value > 0.0)) return LQP_ERR_INVALID;
    return forward_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace,
                         workspace_bytes, 0.0, 0.0, &term);
}

int lqp_boxqp_forward_l1(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                         const void* b, const void* lb, const void* ub, const void* w, const void* c, const lqp_boxqp_ctrl* ctrl,
                         const void* rho_in, void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* side, void* u_box,
                         lqp_boxqp_stats* stats, void* workspace, size_t workspace_bytes) {
    const TermArgs term = {TermL1::kind, {w, c, nullptr, nullptr}, side, u_box};
    return term_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, term, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace, workspace_bytes);
}

int lqp_boxqp_forward_soft(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                           const void* b, const void* lb, const void* ub, const void* wl, const void* wu, const void* lo, const void* hi,
                           const lqp_boxqp_ctrl* ctrl, const void* rho_in, void* x, void* z, void* u, void* lams, void* nus, void* rho_out,
                           void* zone, void* u_box, lqp_boxqp_stats* stats, void* workspace, size_t workspace_bytes) {
    const TermArgs term = {TermSoft::kind, {wl, wu, lo, hi}, zone, u_box};
    return term_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, term, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace, workspace_bytes);
}

int lqp_boxqp_forward_log(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                          const void* b, const void* lb, const void* ub, const void* w, const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                          void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* u_box, void* curv,
                          lqp_boxqp_stats* stats, void* workspace, size_t workspace_bytes) {
    const TermArgs term = {TermLog::kind, {w, nullptr, nullptr, nullptr}, curv, u_box};
    return term_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, term, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace, workspace_bytes);
}

// s: [K + 1][B][n], c: [K][B][n], 1 <= K <= PWL_K.  Fewer kinks than the kernels are written for are padded at the top here, by
// pointers alone: the last slope's vector once more, and no vector (= +inf) for a kink
int lqp_boxqp_forward_pwl(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                          const void* b, const void* lb, const void* ub, const void* s, const void* c, int K, const lqp_boxqp_ctrl* ctrl,
                          const void* rho_in, void* x, void* z, void* u, void* lams, void* nus, void* rho_out, void* piece, void* u_box,
                          lqp_boxqp_stats* stats, void* workspace, size_t workspace_bytes) {
    if (bad_dims(dtype, B, n, m) || !s || !c || K < 1 || K > PWL_K) return LQP_ERR_INVALID;
    const size_t vec = (size_t)B * n * (dtype == LQP_F64 ? 8 : 4);
    TermArgs term;
    term.kind = TermPwl::kind; term.aux = piece; term.u_box = u_box;
    for (int k = 0; k <= PWL_K; ++k) term.in[k] = (const char*)s + (size_t)(k < K ? k : K) * vec;
    for (int k = 0; k < K; ++k) term.in[PWL_K + 1 + k] = (const char*)c + (size_t)k * vec;
    return term_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, term, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace, workspace_bytes);
}

int lqp_boxqp_forward_huber(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                            const void* b, const void* lb, const void* ub, const void* w, const void* c, const void* delta,
                            const lqp_boxqp_ctrl* ctrl, const void* rho_in, void* x, void* z, void* u, void* lams, void* nus, void* rho_out,
                            void* zone, void* u_box, lqp_boxqp_stats* stats, void* workspace, size_t workspace_bytes) {
    const TermArgs term = {TermHuber::kind, {w, c, delta, nullptr}, zone, u_box};
    return term_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, term, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace, workspace_bytes);
}

int lqp_boxqp_l1_effective_box(void* stream, int dtype, int B, int n, const void* side, const void* u, const void* u_box,
                               const void* lb, const void* ub, const void* c, int rho_mode, double rho_value, const void* rho_in,
                               void* lb_e, void* ub_e, void* u_e, void* lams_e) {
    if (!elementwise_ok(dtype, B, n, {side, u, u_box, lb, ub, c, lb_e, ub_e, u_e, lams_e}) || (rho_mode == 2 && !rho_in)) return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_l1_effective_box<T>, grid, dim3(256), 0, st, (const T*)side, (const T*)u, (const T*)u_box, (const T*)lb, (const T*)ub,
                           (const T*)c, rho_mode == 2 ? (const T*)rho_in : nullptr, (T)rho_value, n, total, (T*)lb_e, (T*)ub_e, (T*)u_e, (T*)lams_e);
    });
}

int lqp_boxqp_l1_finish_grads(void* stream, int dtype, int B, int n, const void* side, const void* dp, const void* dlb_e,
                              const void* dub_e, void* dlb, void* dub, void* dc, void* dw) {
    if (!elementwise_ok(dtype, B, n, {side, dp, dlb_e, dub_e})) return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_l1_finish_grads<T>, grid, dim3(256), 0, st, (const T*)side, (const T*)dp, (const T*)dlb_e, (const T*)dub_e, total,
                           (T*)dlb, (T*)dub, (T*)dc, (T*)dw);
    });
}

int lqp_boxqp_soft_effective_box(void* stream, int dtype, int B, int n, const void* zone, const void* u, const void* u_box,
                                 const void* lb, const void* ub, const void* lo, const void* hi, int rho_mode, double rho_value,
                                 const void* rho_in, void* lb_e, void* ub_e, void* u_e, void* lams_e) {
    if (!elementwise_ok(dtype, B, n, {zone, u, u_box, lb, ub, lo, hi, lb_e, ub_e, u_e, lams_e}) || (rho_mode == 2 && !rho_in)) return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_soft_effective_box<T>, grid, dim3(256), 0, st, (const T*)zone, (const T*)u, (const T*)u_box, (const T*)lb, (const T*)ub,
                           (const T*)lo, (const T*)hi, rho_mode == 2 ? (const T*)rho_in : nullptr, (T)rho_value, n, total, (T*)lb_e, (T*)ub_e,
                           (T*)u_e, (T*)lams_e);
    });
}

int lqp_boxqp_soft_finish_grads(void* stream, int dtype, int B, int n, const void* zone, const void* u_box, const void* dp, const void* dlb_e,
                                const void* dub_e, void* dlb, void* dub, void* dwl, void* dwu, void* dlo, void* dhi) {
    if (!elementwise_ok(dtype, B, n, {zone, u_box, dp, dlb_e, dub_e})) return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_soft_finish_grads<T>, grid, dim3(256), 0, st, (const T*)zone, (const T*)u_box, (const T*)dp, (const T*)dlb_e,
                           (const T*)dub_e, total, (T*)dlb, (T*)dub, (T*)dwl, (T*)dwu, (T*)dlo, (T*)dhi);
    });
}

int lqp_boxqp_pwl_effective_box(void* stream, int dtype, int B, int n, const void* piece, const void* u, const void* u_box,
                                const void* lb, const void* ub, const void* c, int K, int rho_mode, double rho_value,
                                const void* rho_in, void* lb_e, void* ub_e, void* u_e, void* lams_e) {
    if (!elementwise_ok(dtype, B, n, {piece, u, u_box, lb, ub, c, lb_e, ub_e, u_e, lams_e}) || (rho_mode == 2 && !rho_in) || K < 1 || K > PWL_K)
        return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_pwl_effective_box<T>, grid, dim3(256), 0, st, (const T*)piece, (const T*)u, (const T*)u_box, (const T*)lb, (const T*)ub,
                           (const T*)c, K, rho_mode == 2 ? (const T*)rho_in : nullptr, (T)rho_value, n, total, (T*)lb_e, (T*)ub_e, (T*)u_e,
                           (T*)lams_e);
    });
}

int lqp_boxqp_pwl_finish_grads(void* stream, int dtype, int B, int n, const void* piece, const void* u_box, const void* dp, const void* dlb_e,
                               const void* dub_e, int K, void* dlb, void* dub, void* ds, void* dc) {
    if (!elementwise_ok(dtype, B, n, {piece, u_box, dp, dlb_e, dub_e}) || K < 1 || K > PWL_K) return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_pwl_finish_grads<T>, grid, dim3(256), 0, st, (const T*)piece, (const T*)u_box, (const T*)dp, (const T*)dlb_e,
                           (const T*)dub_e, K, total, (T*)dlb, (T*)dub, (T*)ds, (T*)dc);
    });
}

int lqp_boxqp_log_effective_duals(void* stream, int dtype, int B, int n, const void* u_box, int rho_mode, double rho_value,
                                  const void* rho_in, void* u_e, void* lams_e) {
    if (!elementwise_ok(dtype, B, n, {u_box, u_e, lams_e}) || (rho_mode != 1 && rho_mode != 2) || (rho_mode == 2 && !rho_in)) return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_log_effective_duals<T>, grid, dim3(256), 0, st, (const T*)u_box, rho_mode == 2 ? (const T*)rho_in : nullptr,
                           (T)rho_value, n, total, (T*)u_e, (T*)lams_e);
    });
}

int lqp_boxqp_log_finish_grads(void* stream, int dtype, int B, int n, const void* dp, const void* z, const void* w, void* dw) {
    if (!elementwise_ok(dtype, B, n, {dp, z, w})) return LQP_ERR_INVALID;
    if (!dw) return LQP_OK;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_log_finish_grads<T>, grid, dim3(256), 0, st, (const T*)dp, (const T*)z, (const T*)w, total, (T*)dw);
    });
}

int lqp_boxqp_huber_effective_duals(void* stream, int dtype, int B, int n, const void* u_box, const void* zone, const void* w,
                                    int rho_mode, double rho_value, const void* rho_in, void* u_e, void* lams_e, void* curv) {
    if (!elementwise_ok(dtype, B, n, {u_box, zone, w, u_e, lams_e, curv}) || (rho_mode != 1 && rho_mode != 2) || (rho_mode == 2 && !rho_in))
        return LQP_ERR_INVALID;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_huber_effective_duals<T>, grid, dim3(256), 0, st, (const T*)u_box, (const T*)zone, (const T*)w,
                           rho_mode == 2 ? (const T*)rho_in : nullptr, (T)rho_value, n, total, (T*)u_e, (T*)lams_e, (T*)curv);
    });
}

int lqp_boxqp_huber_finish_grads(void* stream, int dtype, int B, int n, const void* dp, const void* z, const void* zone, const void* w,
                                 const void* c, const void* delta, void* dw, void* dc, void* ddelta) {
    if (!elementwise_ok(dtype, B, n, {dp, z, zone, w, c, delta})) return LQP_ERR_INVALID;
    if (!dw && !dc && !ddelta) return LQP_OK;
    return elementwise(stream, dtype, B, n, [&](auto t, dim3 grid, hipStream_t st, size_t total) {
        typedef decltype(t) T;
        hipLaunchKernelGGL(k_huber_finish_grads<T>, grid, dim3(256), 0, st, (const T*)dp, (const T*)z, (const T*)zone, (const T*)w, (const T*)c,
                           (const T*)delta, total, (T*)dw, (T*)dc, (T*)ddelta);
    });
}

size_t lqp_boxqp_forward_certify_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { return carve_forward<decltype(t)>(nullptr, B, n, m).bytes_for(FORM_CERTIFY); });
}

int lqp_boxqp_forward_certify(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A,
                              const void* b, const void* lb, const void* ub, const lqp_boxqp_ctrl* ctrl, const void* rho_in,
                              void* x, void* z, void* u, void* lams, void* nus, void* rho_out, lqp_boxqp_stats* stats,
                              void* workspace, size_t workspace_bytes, double eps_prim_inf, double eps_dual_inf) {
    // refused before anything is touched, as lqp_boxqp_forward_detect does: a threshold that is neither 0 (off) nor inside (0, 1)
    // (NaN fails every comparison), both off, no per-problem stop, a check hook, the factor kept for the unroll sweep
    const auto ok = [](double e) { return e == 0.0 || (e > 0.0 && e < 1.0); };
    if (!ok(eps_prim_inf) || !ok(eps_dual_inf) || (eps_prim_inf == 0.0 && eps_dual_inf == 0.0)) return LQP_ERR_INVALID;
    if (!ctrl || !(ctrl->reserved2 & 8) || (ctrl->reserved2 & 1) || ctrl->check_hook) return LQP_ERR_INVALID;
    return forward_entry(stream, dtype, B, n, m, Q, p, A, b, lb, ub, ctrl, rho_in, x, z, u, lams, nus, rho_out, stats, workspace,
                         workspace_bytes, eps_prim_inf, eps_dual_inf);
}

int lqp_boxqp_forward_finish(void* stream, int B, int max_iters, int check_solved, const void* host_report,
                             lqp_boxqp_stats* stats) {
    if (!host_report || !stats || B < 1) return LQP_ERR_INVALID;
    if (stats->mode_used != 4) return LQP_OK;               // (the forward call waited itself)
    const int rc = collect_report((hipStream_t)stream, (const int*)host_report, true, B, max_iters,
                                  check_solved < 1 ? 1 : check_solved, stats);
    return rc == LQP_RETRY_LU ? LQP_ERR_NOT_SPD : rc;
}

// ---- unroll=True: backward through the unrolled loop (the unroll section above) ----
size_t lqp_boxqp_unroll_backward_workspace_bytes(int B, int n, int m, int iters) {
    if (B < 1 || n < 1 || m < 0 || iters < 0) return 0;
    UnrollParams U;
    return carve_tape<float>(nullptr, B, n, m, iters + 1, false, U);
}

int lqp_boxqp_unroll_backward(void* stream, int B, int n, int m, const void* fwd_workspace, size_t fwd_workspace_bytes,
                              int iters, const void* dl_dx, void* dQs, void* dps, void* dAs, void* dbs, void* dlbs,
                              void* dubs, void* drho, void* dD, void* scratch, size_t scratch_bytes) {
    if (B < 1 || n < 1 || m < 0 || iters < 0 || !fwd_workspace || !dl_dx || !dps || !dlbs || !dubs || !drho || !dD || !scratch)
        return LQP_ERR_INVALID;
    if (m > 0 && (!dAs || !dbs)) return LQP_ERR_INVALID;
    UnrollCall c;
    c.st = (hipStream_t)stream; c.B = B; c.n = n; c.m = m; c.iters = iters;
    c.fwd_ws = fwd_workspace; c.fwd_ws_bytes = fwd_workspace_bytes; c.scratch = scratch; c.scratch_bytes = scratch_bytes;
    c.g = dl_dx; c.dQs = dQs; c.dps = dps; c.dAs = dAs; c.dbs = dbs; c.dlbs = dlbs; c.dubs = dubs; c.drho = drho; c.dD = dD;
    return unroll_backward_sym_impl(c);
}

size_t lqp_boxqp_unroll_backward_lu_workspace_bytes(int dtype, int B, int n, int m, int iters) {
    if (bad_dims(dtype, B, n, m) || iters < 0) return 0;
    return by_dtype(dtype, [&](auto t) { UnrollLuParams<decltype(t)> U; return carve_tape<decltype(t)>(nullptr, B, n, m, iters + 1, false, U); });
}

int lqp_boxqp_unroll_backward_lu(void* stream, int dtype, int B, int n, int m, const void* fwd_workspace, size_t fwd_workspace_bytes,
                                 int iters, const void* dl_dx, void* dQs, void* dps, void* dAs, void* dbs, void* dlbs, void* dubs,
                                 void* drho, void* dD, void* scratch, size_t scratch_bytes) {
    if (bad_dims(dtype, B, n, m) || iters < 0 || !fwd_workspace || !dl_dx || !dps || !dlbs || !dubs || !drho || !dD || !scratch)
        return LQP_ERR_INVALID;
    if (m > 0 && (!dAs || !dbs)) return LQP_ERR_INVALID;
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    UnrollCall c;
    c.st = (hipStream_t)stream; c.dtype = dtype; c.B = B; c.n = n; c.m = m; c.iters = iters;
    c.fwd_ws = fwd_workspace; c.fwd_ws_bytes = fwd_workspace_bytes; c.scratch = scratch; c.scratch_bytes = scratch_bytes;
    c.g = dl_dx; c.dQs = dQs; c.dps = dps; c.dAs = dAs; c.dbs = dbs; c.dlbs = dlbs; c.dubs = dubs; c.drho = drho; c.dD = dD;
    return by_dtype(dtype, [&](auto t) { return unroll_backward_lu_impl<decltype(t)>(c); });
}

size_t lqp_boxqp_unroll_tape_workspace_bytes(int dtype, int B, int n, int m, int iters) {
    if (bad_dims(dtype, B, n, m) || iters < 0) return 0;
    return by_dtype(dtype, [&](auto t) { UnrollLuParams<decltype(t)> U; return carve_tape<decltype(t)>(nullptr, B, n, m, iters + 1, true, U); });
}

int lqp_boxqp_unroll_tape_segment(void* stream, int dtype, int B, int n, int m, const void* fwd_workspace, size_t fwd_workspace_bytes,
                                  int iters, int k0, int k1, int mode, const void* packed_buf, const void* rho, void* state, int inj_k,
                                  const void* inj, const void* dl_dx, void* dps, void* dlbs, void* dubs, void* drho, void* dD,
                                  void* scratch, size_t scratch_bytes, void** z_rows, void** u_rows, void** x_rows) {
    if (bad_dims(dtype, B, n, m) || iters < 0 || !fwd_workspace || !scratch || k0 < 0 || k1 > iters + 1 || (mode & ~3) != 0)
        return LQP_ERR_INVALID;
    if (k1 > k0 && (mode & 2) && (!dl_dx || !dps || !dlbs || !dubs || !drho || !dD)) return LQP_ERR_INVALID;
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    UnrollCall c;
    c.st = (hipStream_t)stream; c.dtype = dtype; c.B = B; c.n = n; c.m = m; c.iters = iters;
    c.fwd_ws = fwd_workspace; c.fwd_ws_bytes = fwd_workspace_bytes; c.scratch = scratch; c.scratch_bytes = scratch_bytes;
    c.g = dl_dx; c.dps = dps; c.dlbs = dlbs; c.dubs = dubs; c.drho = drho; c.dD = dD;
    c.k0 = k0; c.k1 = k1; c.mode = mode; c.packed_buf = packed_buf; c.rho = rho; c.state = state; c.inj_k = inj_k; c.inj = inj;
    c.zrows = z_rows; c.urows = u_rows; c.xrows = x_rows;
    return by_dtype(dtype, [&](auto t) { return unroll_tape_segment_impl<decltype(t)>(c); });
}

int lqp_boxqp_unroll_tape_finish(void* stream, int dtype, int B, int n, int m, int iters, void* dQs, void* dAs, void* dbs, void* scratch,
                                 size_t scratch_bytes) {
    if (bad_dims(dtype, B, n, m) || iters < 0 || !scratch || (m > 0 && (!dAs || !dbs))) return LQP_ERR_INVALID;
    UnrollCall c;
    c.st = (hipStream_t)stream; c.dtype = dtype; c.B = B; c.n = n; c.m = m; c.iters = iters;
    c.scratch = scratch; c.scratch_bytes = scratch_bytes; c.dQs = dQs; c.dAs = dAs; c.dbs = dbs;
    return by_dtype(dtype, [&](auto t) { return unroll_tape_finish_impl<decltype(t)>(c); });
}

int lqp_unroll_scale_colmax(void* stream, int B, int n, const void* Q, void* colmax, void* argmax, void* count) {
    if (B < 0 || n < 1 || !Q || !colmax || !argmax || !count) return LQP_ERR_INVALID;
    if (B == 0) return LQP_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, PC_UNROLL_SCALE);
    int dev = 0, cus = 0;
    const int slabs = (current_device_cus(&dev, &cus) && 2 * B <= cus && n >= 128) ? 2 : 1;      // column halves when half the chip is idle
    hipLaunchKernelGGL(k_unroll_scale_colmax<>, dim3(B, slabs), dim3(LQP_NT), 0, st, (const float*)Q, n, (float*)colmax, (int*)argmax, (int*)count);
    return last_error();
}

int lqp_unroll_scale_grad_slabs(int B, int n) {
    (void)n;
    int dev = 0, cus = 0;
    if (B < 1 || !current_device_cus(&dev, &cus)) return 1;
    int s = (8 * cus) / B;                       // 256-thread workgroups: eight per CU fill it
    return s < 1 ? 1 : (s > 32 ? 32 : s);
}

int lqp_unroll_scale_grad(void* stream, int B, int n, const void* Q, const void* d, const void* s, void* G, void* parts, int slabs) {
    if (B < 0 || n < 1 || !Q || !G || !parts || slabs < 1 || slabs > 64) return LQP_ERR_INVALID;
    if (B == 0) return LQP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int lds = 4 * n * (int)sizeof(float);
    if (lds > 64 * 1024) return LQP_ERR_UNSUPPORTED;
    int rc = ensure_lds((const void*)k_unroll_scale_grad<>, lds);
    if (rc) return rc;
    ProfScope ps(st, PC_UNROLL_SCALE);
    hipLaunchKernelGGL(k_unroll_scale_grad<>, dim3(B, slabs), dim3(256), lds, st, (const float*)Q, (const float*)d, (const float*)s,
                       (float*)G, n, (float*)parts);
    return last_error();
}

int lqp_unroll_scale_vectors(void* stream, int B, int n, int m, int phase, int has_box, int beta_given, double beta_value,
                             const void* colmax, const void* p, const void* A, const void* b, const void* lb, const void* ub,
                             const void* g_ps, const void* g_As, const void* g_bs, const void* g_lbs, const void* g_ubs, const void* g_D,
                             const void* parts, int nparts, void* d_out, void* dp, void* dA, void* db, void* dlb, void* dub,
                             void* g_colmax) {
    if (B < 0 || n < 1 || m < 0 || !colmax || (phase != 0 && phase != 1)) return LQP_ERR_INVALID;
    if (phase == 0 && !d_out) return LQP_ERR_INVALID;
    if (phase == 1 && (!p || !g_colmax || (m > 0 && (!A || !b || !g_As)) || (has_box && (!lb || !ub)) || (nparts > 0 && !parts)))
        return LQP_ERR_INVALID;
    if (B == 0) return LQP_OK;
    const int lds = unroll_scale_vectors_lds_bytes(n, m);
    if (lds > 160 * 1024) return LQP_ERR_UNSUPPORTED;
    int rc = ensure_lds((const void*)k_unroll_scale_vectors<>, lds);
    if (rc) return rc;
    ScaleVecParams P;
    memset(&P, 0, sizeof(P));
    P.n = n; P.m = m; P.phase = phase; P.has_box = has_box; P.beta_given = beta_given; P.nparts = nparts; P.beta_value = (float)beta_value;
    P.cn = (const float*)colmax; P.p = (const float*)p; P.A = (const float*)A; P.b = (const float*)b; P.lb = (const float*)lb; P.ub = (const float*)ub;
    P.gps = (const float*)g_ps; P.gAs = (const float*)g_As; P.gbs = (const float*)g_bs; P.glbs = (const float*)g_lbs; P.gubs = (const float*)g_ubs;
    P.gD = (const float*)g_D; P.parts = (const float*)parts;
    P.d_out = (float*)d_out; P.dp = (float*)dp; P.dA = (float*)dA; P.db = (float*)db; P.dlb = (float*)dlb; P.dub = (float*)dub; P.gcn = (float*)g_colmax;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, PC_UNROLL_SCALE);
    hipLaunchKernelGGL(k_unroll_scale_vectors<>, dim3(B), dim3(LQP_NT), lds, st, P);
    return last_error();
}

int lqp_unroll_scale_scatter(void* stream, int B, int n, const void* Q, const void* colmax, const void* argmax, const void* count,
                             const void* g_colmax, void* G) {
    if (B < 0 || n < 1 || !Q || !colmax || !argmax || !count || !g_colmax || !G) return LQP_ERR_INVALID;
    if (B == 0) return LQP_OK;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, PC_UNROLL_SCALE);
    hipLaunchKernelGGL(k_unroll_scale_scatter<>, dim3(B), dim3(LQP_NT), 0, st, (const float*)Q, (const float*)colmax, (const int*)argmax,
                       (const int*)count, (const float*)g_colmax, (float*)G, n);
    return last_error();
}

int lqp_boxqp_last_residuals(void* stream, int dtype, int B, int n, int m, const void* workspace, size_t workspace_bytes,
                             void* primal_out, void* dual_out) {
    if (bad_dims(dtype, B, n, m) || !workspace) return LQP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return LQP_OK;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const FwdLayout<T> L = carve_forward<T>(const_cast<void*>(workspace), B, n, m);
        if (workspace_bytes < L.bytes) return (int)LQP_ERR_WORKSPACE;
        hipLaunchKernelGGL(k_copy_residuals<T>, dim3((B + 255) / 256), dim3(256), 0, st, L.P.scal, (T*)primal_out, (T*)dual_out, B);
        return last_error();
    });
}

int lqp_boxqp_problem_iters(void* stream, int dtype, int B, int n, int m, const void* workspace, size_t workspace_bytes,
                            int32_t* iters_out) {
    if (bad_dims(dtype, B, n, m) || !workspace || !iters_out) return LQP_ERR_INVALID;
    if (!each_ws_known(workspace)) return LQP_ERR_INVALID;      // (the last forward on this workspace did not run with bit 3)
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return LQP_OK;
    const int* src = nullptr;
    const size_t need = by_dtype(dtype, [&](auto t) {
        const FwdLayout<decltype(t)> L = carve_forward<decltype(t)>(const_cast<void*>(workspace), B, n, m);
        src = L.pstat_area;
        return L.bytes;
    });
    if (workspace_bytes < need) return LQP_ERR_WORKSPACE;
    hipLaunchKernelGGL(k_copy_iters<>, dim3((B + 255) / 256), dim3(256), 0, st, src, (int*)iters_out, B);
    return last_error();
}

int lqp_boxqp_problem_status(void* stream, int dtype, int B, int n, int m, const void* workspace, size_t workspace_bytes,
                             int32_t* status_out) {
    if (bad_dims(dtype, B, n, m) || !workspace || !status_out) return LQP_ERR_INVALID;
    if (!each_ws_known(workspace)) return LQP_ERR_INVALID;      // (the last forward on this workspace did not run with bit 3)
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) return LQP_OK;
    const int* src = nullptr;
    const size_t need = by_dtype(dtype, [&](auto t) {
        const FwdLayout<decltype(t)> L = carve_forward<decltype(t)>(const_cast<void*>(workspace), B, n, m);
        src = L.pstat_area;
        return L.bytes;
    });
    if (workspace_bytes < need) return LQP_ERR_WORKSPACE;
    hipLaunchKernelGGL(k_copy_pstatus<>, dim3((B + 255) / 256), dim3(256), 0, st, src, (int*)status_out, B);
    return last_error();
}

int lqp_boxqp_check_trace(void* stream, int dtype, int B, int n, int m, const void* workspace, size_t workspace_bytes,
                          int n_checks, void* trace_out) {
    if (bad_dims(dtype, B, n, m) || !workspace || !trace_out || n_checks < 0) return LQP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 || n_checks == 0) return LQP_OK;
    const unsigned int* src = nullptr;
    const size_t need = by_dtype(dtype, [&](auto t) {
        const FwdLayout<decltype(t)> L = carve_forward<decltype(t)>(const_cast<void*>(workspace), B, n, m);
        src = L.vtrace_area;
        return L.bytes;
    });
    if (workspace_bytes < need) return LQP_ERR_WORKSPACE;
    const int words = 2 * (n_checks < kRing ? n_checks : kRing);
    hipLaunchKernelGGL(k_copy_trace<>, dim3((words + 255) / 256), dim3(256), 0, st, src, (float*)trace_out, words);
    return last_error();
}

size_t lqp_boxqp_backward_fp_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { BwdParams<decltype(t)> P; return carve_backward<decltype(t)>(nullptr, B, n, m, P); });
}

int lqp_boxqp_backward_fp_prefactor(void* stream, int dtype, int B, int n, int m, const void* x, const void* u, const void* Q,
                                    const void* A, const void* lb, const void* ub, void* workspace, size_t workspace_bytes,
                                    int linsolve, void* host_report) {
    if (bad_dims(dtype, B, n, m) || !x || !u || !Q || !lb || !ub || !workspace) return LQP_ERR_INVALID;
    if (m > 0 && !A) return LQP_ERR_INVALID;
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    BwdCall c;
    c.st = (hipStream_t)stream; c.dtype = dtype; c.B = B; c.n = n; c.m = m;
    c.ws = workspace; c.ws_bytes = workspace_bytes; c.linsolve = linsolve == 2 ? 2 : 1; c.host_report = host_report;
    c.x = x; c.u = u; c.Q = Q; c.A = A; c.lb = lb; c.ub = ub;
    c.prefactor = true;
    return backward_call(c);
}

int lqp_boxqp_backward_fp(void* stream, int dtype, int B, int n, int m, const void* dl_dz, const void* x, const void* u,
                          const void* lams, const void* nus, const void* Q, const void* A, const void* lb, const void* ub,
                          int rho_mode, double rho_value, const void* rho_in, void* dQ, void* dp, void* dA, void* db,
                          void* dlb, void* dub, int32_t* fail_index, void* workspace, size_t workspace_bytes, int linsolve,
                          void* host_report) {
    if (bad_dims(dtype, B, n, m) || !dl_dz || !x || !u || !lams || !Q || !lb || !ub || !workspace) return LQP_ERR_INVALID;
    if (m > 0 && (!A || !nus)) return LQP_ERR_INVALID;
    if (rho_mode != 1 && rho_mode != 2) return LQP_ERR_INVALID;
    if (rho_mode == 2 && !rho_in) return LQP_ERR_INVALID;
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    BwdCall c;
    c.st = (hipStream_t)stream; c.dtype = dtype; c.B = B; c.n = n; c.m = m;
    c.ws = workspace; c.ws_bytes = workspace_bytes; c.linsolve = linsolve; c.host_report = host_report;
    c.g = dl_dz; c.x = x; c.u = u; c.lams = lams; c.nus = nus; c.Q = Q; c.A = A; c.lb = lb; c.ub = ub;
    c.rho_mode = rho_mode; c.rho_value = rho_value; c.rho_in = rho_in;
    c.dQ = dQ; c.dp = dp; c.dA = dA; c.db = db; c.dlb = dlb; c.dub = dub; c.fail_index = fail_index;
    return backward_call(c);
}

int lqp_boxqp_backward_fp_curv(void* stream, int dtype, int B, int n, int m, const void* dl_dz, const void* x, const void* u,
                               const void* lams, const void* nus, const void* Q, const void* A, const void* lb, const void* ub,
                               const void* curv, int rho_mode, double rho_value, const void* rho_in, void* dQ, void* dp, void* dA,
                               void* db, void* dlb, void* dub, int32_t* fail_index, void* workspace, size_t workspace_bytes,
                               int linsolve, void* host_report) {
    if (bad_dims(dtype, B, n, m) || !dl_dz || !x || !u || !lams || !Q || !lb || !ub || !workspace) return LQP_ERR_INVALID;
    if (m > 0 && (!A || !nus)) return LQP_ERR_INVALID;
    if (rho_mode != 1 && rho_mode != 2) return LQP_ERR_INVALID;
    if (rho_mode == 2 && !rho_in) return LQP_ERR_INVALID;
    if (linsolve & LQP_BWD_PREFACTORED) return LQP_ERR_INVALID;      // (no prefactor phase carries the diagonal)
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    BwdCall c;
    c.st = (hipStream_t)stream; c.dtype = dtype; c.B = B; c.n = n; c.m = m;
    c.ws = workspace; c.ws_bytes = workspace_bytes; c.linsolve = linsolve; c.host_report = host_report;
    c.g = dl_dz; c.x = x; c.u = u; c.lams = lams; c.nus = nus; c.Q = Q; c.A = A; c.lb = lb; c.ub = ub; c.curv = curv;
    c.rho_mode = rho_mode; c.rho_value = rho_value; c.rho_in = rho_in;
    c.dQ = dQ; c.dp = dp; c.dA = dA; c.db = db; c.dlb = dlb; c.dub = dub; c.fail_index = fail_index;
    return backward_call(c);
}

int lqp_boxqp_backward_kkt(void* stream, int dtype, int B, int n, int m, const void* dl_dz, const void* x,
                           const void* lams, const void* nus, const void* Q, const void* A, const void* lb, const void* ub,
                           void* dQ, void* dp, void* dA, void* db, void* dlb, void* dub, int32_t* fail_index, void* workspace,
                           size_t workspace_bytes, int linsolve, void* host_report) {
    if (bad_dims(dtype, B, n, m) || !dl_dz || !x || !lams || !Q || !lb || !ub || !workspace) return LQP_ERR_INVALID;
    if (m > 0 && (!A || !nus)) return LQP_ERR_INVALID;
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    BwdCall c;
    c.st = (hipStream_t)stream; c.dtype = dtype; c.B = B; c.n = n; c.m = m;
    c.ws = workspace; c.ws_bytes = workspace_bytes; c.linsolve = linsolve; c.host_report = host_report;
    c.g = dl_dz; c.x = x; c.lams = lams; c.nus = nus; c.Q = Q; c.A = A; c.lb = lb; c.ub = ub;
    c.dQ = dQ; c.dp = dp; c.dA = dA; c.db = db; c.dlb = dlb; c.dub = dub; c.fail_index = fail_index;
    c.kkt = true;
    return backward_call(c);
}

size_t lqp_spd_inverse_workspace_bytes(int dtype, int B, int n) {
    if (dtype != LQP_F32 || B < 0 || n < 1) return 0;
    const int Ks = round_up(n, LQP_NB) / LQP_NB;
    // (above 512: + the panel scratch of wg_spd_sweep_big)
    return (size_t)B * (sym_blocks(Ks) + (Ks > SPD_MAXK ? Ks - 1 : 0)) * LQP_BLK * sizeof(float) + 2 * kAlign;
}

int lqp_spd_inverse_batched(void* stream, int dtype, int B, int n, const void* K_in, void* Kinv_out, int32_t* info_out,
                            void* workspace, size_t workspace_bytes) {
    if (dtype != LQP_F32) return LQP_ERR_UNSUPPORTED;
    if (B < 0 || n < 1 || !K_in || !Kinv_out || !info_out || !workspace) return LQP_ERR_INVALID;
    const int Ks = round_up(n, LQP_NB) / LQP_NB;
    if (Ks > SPD_BIGK) return LQP_ERR_UNSUPPORTED;
    if (workspace_bytes < lqp_spd_inverse_workspace_bytes(dtype, B, n)) return LQP_ERR_WORKSPACE;
    if (B == 0) return LQP_OK;
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace);
    float* Hs = c.take<float>((size_t)B * sym_blocks(Ks) * LQP_BLK);
    float* Yg = Ks > SPD_MAXK ? c.take<float>((size_t)B * (Ks - 1) * LQP_BLK) : nullptr;
    const int lds = spd_lds_bytes(Ks > SPD_MAXK ? SPD_MAXK : Ks);
    auto dense_fn = Ks > SPD_MAXK ? k_spd_inverse_dense<2> : k_spd_inverse_dense<1>;
    int rc = ensure_lds((const void*)dense_fn, lds);
    if (rc) return rc;
    { ProfScope ps(st, PC_SPD_INV);
      hipLaunchKernelGGL(dense_fn, dim3(B), dim3(LQP_NT), lds, st, (const float*)K_in, (float*)Kinv_out, Hs,
                         (int*)info_out, n, Ks, Yg); }
    return last_error();
}

size_t lqp_lu_factor_workspace_bytes(int dtype, int B, int N) {
    if (bad_dims(dtype, B, N, 0)) return 0;
    int* piv; unsigned long long* scr;
    return by_dtype(dtype, [&](auto t) { decltype(t)* M; return carve_lu<decltype(t)>(nullptr, B, N, M, piv, scr); });
}

int lqp_lu_factor_batched(void* stream, int dtype, int B, int N, void* M_inout, int32_t* piv_out, int32_t* info_out,
                          void* workspace, size_t workspace_bytes) {
    if (bad_dims(dtype, B, N, 0) || !M_inout || !piv_out || !info_out || !workspace) return LQP_ERR_INVALID;
    if (N > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) { return lu_factor_impl<decltype(t)>(st, B, N, M_inout, piv_out, info_out, workspace, workspace_bytes); });
}

size_t lqp_lu_packed_bytes(int dtype, int B, int N) {
    if (bad_dims(dtype, B, N, 0)) return 0;
    return by_dtype(dtype, [&](auto t) { return packed_bytes_t<decltype(t)>(B, N); });
}
size_t lqp_lu_solve_workspace_bytes(int dtype, int B, int N) { return lqp_lu_packed_bytes(dtype, B, N); }

int lqp_lu_pack(void* stream, int dtype, int B, int N, const void* LU, const int32_t* piv, void* packed) {
    if (bad_dims(dtype, B, N, 0) || !LU || !piv || !packed) return LQP_ERR_INVALID;
    if (N > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) { return lu_pack_impl<decltype(t)>(st, B, N, LU, piv, packed); });
}

int lqp_lu_solve_packed(void* stream, int dtype, int B, int N, int k, const void* packed, void* rhs_inout) {
    if (bad_dims(dtype, B, N, 0) || k < 1 || !packed || !rhs_inout) return LQP_ERR_INVALID;
    if (N > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) { return lu_solve_packed_impl<decltype(t)>(st, B, N, k, packed, rhs_inout); });
}

int lqp_lu_solve_batched(void* stream, int dtype, int B, int N, int k, const void* LU, const int32_t* piv, void* rhs_inout,
                         void* workspace, size_t workspace_bytes) {
    if (!workspace || workspace_bytes < lqp_lu_packed_bytes(dtype, B, N)) return workspace ? LQP_ERR_WORKSPACE : LQP_ERR_INVALID;
    int rc = lqp_lu_pack(stream, dtype, B, N, LU, piv, workspace);
    if (rc) return rc;
    return lqp_lu_solve_packed(stream, dtype, B, N, k, workspace, rhs_inout);
}

size_t lqp_kkt_solve_workspace_bytes(int dtype, int B, int n, int m) {
    if (bad_dims(dtype, B, n, m)) return 0;
    return by_dtype(dtype, [&](auto t) { BwdParams<decltype(t)> P; return carve_backward<decltype(t)>(nullptr, B, n, m, P, true); });
}

int lqp_kkt_solve(void* stream, int dtype, int B, int n, int m, const void* Q, const void* p, const void* A, const void* b,
                  void* x, void* nus, int32_t* fail_index, void* workspace, size_t workspace_bytes) {
    if (bad_dims(dtype, B, n, m) || !Q || !p || !x || !workspace) return LQP_ERR_INVALID;
    if (m > 0 && (!A || !b || !nus)) return LQP_ERR_INVALID;
    if (n + m > max_rows(dtype)) return LQP_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) { return kkt_solve_impl<decltype(t)>(st, B, n, m, Q, p, A, b, x, nus, fail_index, workspace, workspace_bytes); });
}

int lqp_qp_outer_grads(void* stream, int dtype, int B, int n, int m, const void* dx, const void* x, const void* dnu,
                       const void* nus, void* dQ, void* dA) {
    if (bad_dims(dtype, B, n, m) || !dx || !x) return LQP_ERR_INVALID;
    if (m > 0 && dA && (!dnu || !nus)) return LQP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_outer_grads<T>, dim3(B), dim3(LQP_NT), 0, st, (const T*)dx, (const T*)x, (const T*)dnu, (const T*)nus, n, m,
                           (T*)dQ, (T*)dA);
    });
    return last_error();
}

}  // extern "C"
