// libdapol_hip.so -- C ABI (include/dapol_hip.h) over the gfx950 kernels.  Host side only orchestrates: every
// byte of arithmetic (generator derivation included) runs on the GPU; there is no CPU fallback.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>          // radix sort only (plain library plumbing for the leaf-derivation sorts)
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dapol_hip.h"
#include "kernels_ctx_tree.h"
#include "kernels_range.h"
#include "kernels_range_gs.h"
#include "kernels_verify.h"
#include "kernels_leaf.h"
#include "kernels_shared.h"
#include "kernels_verify_shared.h"
#include "kernels_verify_compact.h"
#include "kernels_reprove.h"
#include "kernels_store.h"
#include "kernels_compact_paths.h"
#include "kernels_batches.h"
#include "kernels_reprove_batches.h"
#include "kernels_batch_store.h"

using namespace dapol;

static thread_local std::string g_last_error;
static int32_t fail_hip(hipError_t e, const char* what, const char* file, int line) {
    char buf[256];
    const char* base = strrchr(file, '/');
    snprintf(buf, sizeof buf, "%s failed at %s:%d: %s", what, base ? base + 1 : file, line, hipGetErrorString(e));
    g_last_error = buf;
    // Several entry points fork work onto the context's side streams (chunks in flight, the verifier's own-point ladders, the
    // leaves' commitments of a small tree) and join it later; an error return in between must not leave that work running on the
    // context's scratch, which the next call re-uses without any ordering against those streams.  Errors are rare: drain the device.
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? DAPOL_ERR_OUT_OF_MEMORY : DAPOL_ERR_HIP;
}
static int32_t fail(int32_t code, const char* msg) {
    g_last_error = msg;
    return code;
}
#define HIPCHK(x)                                                  \
    do {                                                           \
        hipError_t e_ = (x);                                       \
        if (e_ != hipSuccess) return fail_hip(e_, #x, __FILE__, __LINE__); \
    } while (0)
#define LAUNCH_CHECK() HIPCHK(hipGetLastError())
// A step that reports with a DAPOL_* code of its own: anything but DAPOL_OK ends the caller with it.
#define RCCHK(x)                   \
    do {                           \
        int32_t rc_ = (x);         \
        if (rc_) return rc_;       \
    } while (0)

// The DAPOL_* environment variables are measurement knobs (A/B switches of tools/ and tests/).  They are read only when the
// process has opted in -- DAPOL_ENV_KNOBS set to anything but "0", or dapol_env_knobs(1) -- so that a host embedding the library
// does not inherit behaviour from stray variables; what an embedder may want to set is a field of dapol_options.
static std::atomic<int> g_env_knobs{-1};          // -1: ask the environment
static std::atomic<unsigned long long> g_fork_guard_waits{0};   // side streams a ForkGuard had to wait for (early returns between fork and join)
static const char* knob(const char* name) {
    int on = g_env_knobs.load(std::memory_order_relaxed);
    if (on < 0) {
        const char* e = getenv("DAPOL_ENV_KNOBS");
        on = (e && *e && strcmp(e, "0") != 0) ? 1 : 0;
    }
    return on ? getenv(name) : nullptr;
}
// Fault injection and limit overrides that exist for tests/ only (DAPOL_TEST_FAIL_AFTER_FORK, DAPOL_TEST_FAIL_UPDATE_MIDWAY / _REMOVE_MIDWAY / _INSERT_MIDWAY,
// DAPOL_LEAF_MAX_TRIES, DAPOL_VSHARED_FORWARD_MAX: they make healthy calls fail, or change when DapolError::FailedToMapIndex fires) need a SECOND opt-in,
// DAPOL_TEST_HOOKS=1, read once per process: the measurement scripts of tools/ export DAPOL_ENV_KNOBS alone and can never trip them,
// and a call site costs a flag test instead of a getenv + strcmp (round-4 advisor).
static const char* test_knob(const char* name) {
    static const bool hooks = [] { const char* e = getenv("DAPOL_TEST_HOOKS"); return e && !strcmp(e, "1"); }();
    return hooks ? knob(name) : nullptr;
}
int32_t dapol_env_knobs(int32_t enable) {
    int old = g_env_knobs.exchange(enable ? 1 : 0);
    if (old < 0) { const char* e = getenv("DAPOL_ENV_KNOBS"); old = (e && *e && strcmp(e, "0") != 0) ? 1 : 0; }
    return old;
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        return hipMalloc((void**)&p, count * sizeof(T));
    }
};

// Launches of the kernels that hash nodes.  They are templates over DX (hash.h: "SHA-256 and SHA3-256"); K names the instantiation
// with DX in it, in parentheses -- (k_tree_merge<1, DX>) -- and DX is DG_SHA256 / DG_SHA3_256 on a context of that digest and
// DG_RUNTIME on every other one.  The rest is hipLaunchKernelGGL's argument list.
#define DX_UNPAREN(...) __VA_ARGS__
#define LAUNCH_DX_AS(V, K, ...)                                              \
    {                                                                        \
        constexpr int DX = V;                                                \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(DX_UNPAREN K), __VA_ARGS__);      \
    }
#define LAUNCH_DX(dg, K, ...)                                                \
    do {                                                                     \
        switch (dg) {                                                        \
            case DG_SHA256: LAUNCH_DX_AS(DG_SHA256, K, __VA_ARGS__) break;   \
            case DG_SHA3_256: LAUNCH_DX_AS(DG_SHA3_256, K, __VA_ARGS__) break; \
            default: LAUNCH_DX_AS(DG_RUNTIME, K, __VA_ARGS__)                \
        }                                                                    \
    } while (0)

static inline unsigned nblk(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

#include "wire_scope.inc"

// ------------------------------------------------------------------------------------------------ context
struct dapol_ctx {
    // One reference for the caller's handle plus one per tree / workload built on the context: dapol_ctx_destroy only
    // drops the caller's, so handles may be destroyed in any order (garbage-collected language bindings do exactly that).
    std::atomic<int> refs{1};
    dapol_options opt{};                                 // zeros = the library's own choices (dapol_ctx_set_options)
    int device = 0;
    int max_parties = 0;
    int n_cu = 256;                                      // hipDeviceProp_t::multiProcessorCount (MI355X: 256)
    int msm_waves_per_cu = 4 * DAPOL_MSM_OCC;            // resident wavefronts of k_rp_msm per CU (occupancy API, dapol_ctx_create)
    // wavefronts the dominant kernel keeps resident on the chip: launches are sized in whole rounds of this many
    size_t resident_waves() const { return (size_t)n_cu * (size_t)msm_waves_per_cu; }
    hipStream_t stream = nullptr;
    hipStream_t side[3] = {nullptr, nullptr, nullptr};   // further pipelines of the range prover (several chunks in flight)
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_v[4] = {nullptr, nullptr, nullptr, nullptr};   // the verifier's commitments landing in column blocks (host_verify.inc: VArrival)
    DevBuf<int32_t> table;       // window tables
    DevBuf<uint32_t> gens_comp;  // compressed base points of every row (for dapol_ctx_generator)
    TableView tv{};
    RangeScratch scratch;        // grown on demand by the range prover
    RangeScratch vio;            // dapol_range_verify_batch's device copies of the caller's proofs / commitments / verdicts: kept between calls
                                 // (a 34 MB hipMalloc + hipFree per call is a few hundred microseconds of a 7 ms pass; at most 1 GB is kept)
    // LANES for the sub-proofs of ONE small call (round 6, host_policy.inc: prove_policy_device): a policy's plan with several groups
    // of sub-proofs -- splitting at height 24 is a 16-party and an 8-party proof, benches/dapol.rs:71-78 -- is latency-bound, and its
    // groups are independent statements; each extra group runs on a lane of its own: a shallow context that shares the tables (tv)
    // and owns its streams, events and scratch.  Made on first use, freed with the context.
    dapol_ctx* aux[3] = {nullptr, nullptr, nullptr};
    uint32_t* h_pinned = nullptr;    // 16 page-locked words: a device-to-host copy into pageable memory blocks the host until the stream has
                                     // drained, which would serialise the lanes; into this it is queued like a kernel
};

// Width of the context's node hash D: 8 words (BLAKE3, Blake2s, SHA-256, SHA3-256) or 16 (Blake2b).  Every H buffer of the C ABI holds this many
// bytes per node (dapol_ctx_digest_bytes).
static inline int ctx_hw(const dapol_ctx* c) { return dg_hash_words(c->tv.digest); }
static inline size_t ctx_hash_bytes(const dapol_ctx* c) { return (size_t)ctx_hw(c) * 4; }
static inline bool ctx_wide(const dapol_ctx* c) { return ctx_hw(c) == 16; }
// Paths that exist for the 32-byte digests only (the sharded / workload / record paths and Dapol::new's leaf derivation, which the
// reference itself refuses for other sizes, src/dapol/mod.rs:101-103).
#define NEEDS_32_BYTE_DIGEST(ctx, what)                                                                                                  \
    do {                                                                                                                                 \
        if (ctx_wide(ctx)) return fail(DAPOL_ERR_INVALID_DIGEST_SIZE, what " needs a 32-byte node digest (DapolError::InvalidDigestSize)"); \
    } while (0)
int32_t dapol_ctx_digest_bytes(dapol_ctx* ctx, int32_t* bytes) {
    if (!ctx || !bytes) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *bytes = (int32_t)ctx_hash_bytes(ctx);
    return DAPOL_OK;
}

const char* dapol_strerror(int32_t code) {
    switch (code) {
        case DAPOL_OK: return "ok";
        case DAPOL_ERR_TREE_HEIGHT_TOO_BIG: return "DAPOL tree height must not exceed 64";
        case DAPOL_ERR_SPARSITY_TOO_SMALL: return "tree height too small for the liability set (2^height < 2n)";
        case DAPOL_ERR_INVALID_DIGEST_SIZE: return "digest size must be 32 bytes";
        case DAPOL_ERR_DUPLICATED_INTERNAL_ID: return "liability set contains a duplicated internal ID";
        case DAPOL_ERR_FAILED_TO_MAP_INDEX: return "failed to map audit ID to a tree index within 128 tries";
        case DAPOL_ERR_BYTES_NOT_ENOUGH: return "decoding: bytes not enough";
        case DAPOL_ERR_VALUE_DECODING: return "decoding: value decoding error";
        case DAPOL_ERR_INVALID_ARGUMENT: return "invalid argument";
        case DAPOL_ERR_UNKNOWN_LEAF: return "no liability at the requested leaf";
        case DAPOL_ERR_NO_DEVICE: return "no usable HIP device (the proving path has no CPU fallback)";
        case DAPOL_ERR_HIP: return "HIP runtime error";
        case DAPOL_ERR_OUT_OF_MEMORY: return "out of device memory";
        case DAPOL_ERR_COMM: return "RCCL error";
        default: return "unknown status";
    }
}
const char* dapol_last_error(void) { return g_last_error.c_str(); }

static bool options_ok(const dapol_options* o) {
    if (!o) return true;
    if (o->struct_size != 0 && o->struct_size != (int32_t)sizeof(dapol_options)) return false;
    if (o->window_bits && (o->window_bits < WBITS_MIN || o->window_bits > WBITS_MAX)) return false;
    if (o->gs_tile_rows && (o->gs_tile_rows < 4 || o->gs_tile_rows % 4)) return false;
    if (o->streams < 0 || o->streams > 4 || o->chunk_proofs < 0 || o->table_gb < 0 || o->scratch_gb < 0) return false;
    if (o->tail_length && o->tail_length != -1 && o->tail_length != 32 && o->tail_length != 64 && o->tail_length != 128 && o->tail_length != 256) return false;
    if (o->small_call_max < 0 || o->verify_batch_min < 0 || o->update_incremental_max < -1) return false;
    if (o->gs_slices != 0 && o->gs_slices != 1 && o->gs_slices != 2 && o->gs_slices != 4 && o->gs_slices != 8 && o->gs_slices != 16) return false;
    if (o->profile != DAPOL_PROFILE_BENCH && o->profile != DAPOL_PROFILE_HOST) return false;
    return true;
}
static int32_t ctx_make_streams(dapol_ctx* c) {
    HIPCHK(hipHostMalloc((void**)&c->h_pinned, 64, hipHostMallocDefault));
    HIPCHK(hipStreamCreate(&c->stream));
    HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < 3; i++) {
        HIPCHK(hipStreamCreate(&c->side[i]));
        HIPCHK(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
    }
    for (int i = 0; i < 4; i++) HIPCHK(hipEventCreateWithFlags(&c->ev_v[i], hipEventDisableTiming));
    return DAPOL_OK;
}
static void ctx_free_streams(dapol_ctx* ctx) {
    if (ctx->h_pinned) { (void)hipHostFree(ctx->h_pinned); ctx->h_pinned = nullptr; }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (int i = 0; i < 3; i++) {
        if (ctx->side[i]) (void)hipStreamDestroy(ctx->side[i]);
        if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    for (int i = 0; i < 4; i++) if (ctx->ev_v[i]) (void)hipEventDestroy(ctx->ev_v[i]);
}
// Lane i (0 = the context itself) for one group of a small call's sub-proofs: see dapol_ctx::aux.
static int32_t ctx_lane(dapol_ctx* ctx, int i, dapol_ctx** out) {
    if (i == 0) { *out = ctx; return DAPOL_OK; }
    dapol_ctx*& a = ctx->aux[i - 1];
    if (!a) {
        dapol_ctx* n = new dapol_ctx();
        n->opt = ctx->opt; n->device = ctx->device; n->max_parties = ctx->max_parties; n->n_cu = ctx->n_cu;
        n->msm_waves_per_cu = ctx->msm_waves_per_cu;
        n->tv = ctx->tv;                                  // the same tables: only the primary owns (and frees) them
        int32_t rc = ctx_make_streams(n);
        if (rc) { ctx_free_streams(n); delete n; return rc; }
        a = n;
    }
    a->opt = ctx->opt;                                    // (dapol_ctx_set_options may have changed since the lane was made)
    *out = a;
    return DAPOL_OK;
}

// A FORK hands kernels that read and write the context's scratch (or a call's own buffers) to a side stream; the matching JOIN makes
// the context's stream wait for them.  An early return between the two -- any HIPCHK / LAUNCH_CHECK -- would leave those kernels
// running while the caller's next call reuses the scratch, or after the call's buffers are freed.  This guard, one per forking
// function, waits for every side stream that was forked and not yet joined when the function is left.  (Nothing to wait for on the
// normal path: the join has closed it.)
struct ForkGuard {
    dapol_ctx* c;
    bool open[3] = {false, false, false};
    explicit ForkGuard(dapol_ctx* c_) : c(c_) {}
    ForkGuard(const ForkGuard&) = delete;
    ForkGuard& operator=(const ForkGuard&) = delete;
    void forked(int i) { open[i] = true; }
    void joined(int i) { open[i] = false; }
    ~ForkGuard() {
        for (int i = 0; i < 3; i++)
            if (open[i]) { (void)hipStreamSynchronize(c->side[i]); g_fork_guard_waits.fetch_add(1, std::memory_order_relaxed); }
    }
};
// Test knob (behind BOTH opt-ins, test_knob above): DAPOL_TEST_FAIL_AFTER_FORK=<site> makes the named site return an error right
// after its fork, as a failed launch would -- tests/test_gpu_fault_paths.py then checks that the next call on the context is clean.
#define FAULT_AFTER_FORK(site)                                                                                          \
    do {                                                                                                                \
        const char* e_ = test_knob("DAPOL_TEST_FAIL_AFTER_FORK");                                                         \
        if (e_ && !strcmp(e_, site)) return fail(DAPOL_ERR_HIP, "injected failure after the fork at " site " (test knob)"); \
    } while (0)

// Combined (random-linear-combination) verification checks that FAILED and went on to bisection / the proof-by-proof check.  On
// batches of valid proofs this stays 0; a test that verifies two different all-valid batches back to back asserts exactly that
// (a stale-scratch dependence between passes shows up as a spurious failure here long before it shows up in a verdict).
static std::atomic<unsigned long long> g_verify_fallbacks{0};
int32_t dapol_diag_verify_fallbacks(uint64_t* count) {
    if (!count) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *count = g_verify_fallbacks.load(std::memory_order_relaxed);
    return DAPOL_OK;
}
// Device time of the proving pipeline of the last dapol_range_prove_batch (HIP events on the context's stream around
// range_prove_device: inputs already in HBM, proofs not yet copied back) -- what tools/bench_small_parties.py quotes.
static std::atomic<double> g_last_range_prove_ms{0.0};
int32_t dapol_diag_range_prove_ms(double* ms) {
    if (!ms) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *ms = g_last_range_prove_ms.load(std::memory_order_relaxed);
    return DAPOL_OK;
}
int32_t dapol_diag_fork_guard_waits(uint64_t* count) {
    if (!count) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *count = g_fork_guard_waits.load(std::memory_order_relaxed);
    return DAPOL_OK;
}

int32_t dapol_ctx_create(int32_t device, int32_t max_parties, int32_t digest_id, dapol_ctx** out) {
    return dapol_ctx_create_opts(device, max_parties, digest_id, nullptr, out);
}
int32_t dapol_ctx_get_options(dapol_ctx* ctx, dapol_options* out) {
    if (!ctx || !out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *out = ctx->opt;
    out->struct_size = (int32_t)sizeof(dapol_options);
    out->window_bits = ctx->tv.wbits;
    out->high_half_rows = ctx->tv.hi_split ? 1 : -1;
    return DAPOL_OK;
}
int32_t dapol_ctx_set_options(dapol_ctx* ctx, const dapol_options* o) {
    if (!ctx || !o) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (!options_ok(o)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad dapol_options (struct_size, or a field out of range)");
    const dapol_options keep = ctx->opt;
    ctx->opt = *o;
    ctx->opt.window_bits = keep.window_bits; ctx->opt.table_gb = keep.table_gb; ctx->opt.high_half_rows = keep.high_half_rows;    // fixed at creation
    ctx->opt.profile = keep.profile;
    return DAPOL_OK;
}
int32_t dapol_ctx_create_opts(int32_t device, int32_t max_parties, int32_t digest_id, const dapol_options* options, dapol_ctx** out) {
    if (!out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (!options_ok(options)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad dapol_options (struct_size, or a field out of range)");
    if (digest_id != DAPOL_DIGEST_BLAKE3 && digest_id != DAPOL_DIGEST_BLAKE2S && digest_id != DAPOL_DIGEST_BLAKE2B && digest_id != DAPOL_DIGEST_SHA256 &&
        digest_id != DAPOL_DIGEST_SHA3_256)
        return fail(DAPOL_ERR_INVALID_DIGEST_SIZE, "node digest must be BLAKE3, Blake2s-256, Blake2b-512, SHA-256 or SHA3-256");
    if (max_parties < 1 || max_parties > 1024 || (max_parties & (max_parties - 1)))
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "max_parties must be a power of two in [1, 1024]");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
        return fail(DAPOL_ERR_NO_DEVICE, "no usable HIP device");
    HIPCHK(hipSetDevice(device));
    dapol_ctx* c = new dapol_ctx();
    if (options) c->opt = *options;
    c->device = device;
    c->max_parties = max_parties;
    {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        if (prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
        // Residency of the dominant kernel (one wavefront per block): what its registers and LDS allow -- asked of the runtime,
        // not assumed.
        int blocks = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_rp_msm<MSM_PLAIN, 4>, 64, 0) == hipSuccess && blocks > 0)
            c->msm_waves_per_cu = blocks;
        else (void)hipGetLastError();
    }
    struct Guard { dapol_ctx* c; ~Guard() { if (c) dapol_ctx_destroy(c); } } guard{c};
    RCCHK(ctx_make_streams(c));
    const int P = max_parties;
    // window width: the widest (<= 17 bits: wider measured slower, profiles/r01_wbits_ab4.txt) whose tables fit the budget --
    // DAPOL_TABLE_GB if set, else 40 GB but never more than 30 % of the memory that is free right now (a second context on
    // the same GPU, or a smaller device, gets narrower windows instead of an allocation failure) -- or DAPOL_WBITS (up to 20)
    int wbits = WBITS_MIN;
    {
        const char* eb = knob("DAPOL_TABLE_GB");
        double budget = 40.0e9;
        size_t free_b = 0, total_b = 0;
        if (c->opt.profile == DAPOL_PROFILE_HOST) budget = 18.0e9;       // 16-bit windows for 32 parties (17.3 GB), 15-bit for 64
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)free_b * 0.30 < budget) budget = (double)free_b * 0.30;
        if (c->opt.table_gb > 0) budget = c->opt.table_gb * 1e9;
        if (eb) budget = atof(eb) * 1e9;
        for (int w = WBITS_MIN; w <= WBITS_AUTO_MAX; w++) {
            TableView t{nullptr, P, w, 0, 0};
            if ((double)t.n_rows() * (double)t.row_words() * 4.0 <= budget) wbits = w;
        }
        const char* ew = knob("DAPOL_WBITS");
        if (c->opt.window_bits) wbits = c->opt.window_bits;
        if (ew) {
            int w = atoi(ew);
            if (w < WBITS_MIN || w > WBITS_MAX) return fail(DAPOL_ERR_INVALID_ARGUMENT, "DAPOL_WBITS must be in [8, 20]");
            wbits = w;
        }
    }
    TableView tv{nullptr, P, wbits, digest_id, 0};
    const int rows = tv.n_rows();
    {   // High-half rows for the G / H generators (tables.h): worth their memory (as much again as the G / H rows) only for the
        // prover's materialisation step, so only when they fit beside everything else: DAPOL_TABLE_HI=0 / 1 forces, default = on
        // when the doubled tables stay below 30 % of the free memory and the context is a prover's (<= 64 parties).  Measured
        // interleaved (profiles/r02_hi_rows_ab.txt): +0.7 % at 2^18 proofs, +1.5 % at 2^20, for 34 GB more of HBM.
        size_t free_b = 0, total_b = 0;
        const double bytes2 = (double)(rows + 128 * P) * (double)tv.row_words() * 4.0;
        bool hi = P <= 64 && hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes2 <= 0.30 * (double)free_b;
        if (c->opt.profile == DAPOL_PROFILE_HOST) hi = false;             // as much memory again for +1.5-2 %: not for a shared GPU
        if (c->opt.high_half_rows) hi = c->opt.high_half_rows > 0 && P <= 64;
        if (const char* e = knob("DAPOL_TABLE_HI")) hi = atoi(e) != 0;
        if (hi) tv.hi_split = (tv.nwin_c() + 1) / 2;
    }
    const int rows_total = tv.n_rows_total();
    DevBuf<uint32_t> uniform;
    DevBuf<int32_t> base_pts;
    HIPCHK(uniform.alloc((size_t)2 * P * 64 * 16));
    HIPCHK(base_pts.alloc((size_t)rows_total * 40));
    HIPCHK(c->table.alloc((size_t)rows_total * tv.row_words()));
    HIPCHK(c->gens_comp.alloc((size_t)rows * 8));
    hipLaunchKernelGGL(k_ctx_chains, dim3(nblk(2 * P, 64)), dim3(64), 0, c->stream, uniform.p, P);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ctx_points, dim3(nblk(128 * P, 64)), dim3(64), 0, c->stream, base_pts.p, uniform.p, P);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ctx_pedersen, dim3(1), dim3(64), 0, c->stream, base_pts.p, P, wbits, tv.nwin());
    LAUNCH_CHECK();
    if (tv.hi_split) {
        hipLaunchKernelGGL(k_ctx_hi_points, dim3(nblk(128 * P, 64)), dim3(64), 0, c->stream, base_pts.p, 128 * P, rows, wbits * tv.hi_split);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ctx_table, dim3(nblk((size_t)rows_total * tv.entries(), 64)), dim3(64), 0, c->stream, c->table.p, base_pts.p, rows_total, wbits,
                       tv.entries());
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ctx_compress, dim3(nblk(rows, 64)), dim3(64), 0, c->stream, c->gens_comp.p, base_pts.p, rows);
    LAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tv = tv;
    c->tv.base = c->table.p;
    guard.c = nullptr;
    *out = c;
    return DAPOL_OK;
}

static void ctx_retain(dapol_ctx* ctx) { ctx->refs.fetch_add(1); }
int32_t dapol_ctx_destroy(dapol_ctx* ctx) {
    if (!ctx) return DAPOL_OK;
    if (ctx->refs.fetch_sub(1) > 1) return DAPOL_OK;          // trees / workloads still use it: the last of them frees it
    (void)hipSetDevice(ctx->device);
    for (int i = 0; i < 3; i++)
        if (ctx->aux[i]) {
            ctx->aux[i]->scratch.release();
            ctx->aux[i]->vio.release();
            ctx_free_streams(ctx->aux[i]);
            delete ctx->aux[i];
            ctx->aux[i] = nullptr;
        }
    ctx->scratch.release();
    ctx->vio.release();
    ctx->table.release();
    ctx->gens_comp.release();
    ctx_free_streams(ctx);
    delete ctx;
    return DAPOL_OK;
}

int32_t dapol_ctx_generator(dapol_ctx* ctx, int32_t which, int32_t party, int32_t bit, uint8_t out32[32]) {
    if (!ctx || !out32) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    int row;
    if (which == 0) row = ctx->tv.row_B(0);
    else if (which == 1) row = ctx->tv.row_Bb(0);
    else if ((which == 2 || which == 3) && party >= 0 && party < ctx->max_parties && bit >= 0 && bit < 64)
        row = which == 2 ? ctx->tv.row_G(party, bit) : ctx->tv.row_H(party, bit);
    else return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad generator selector");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpy(out32, ctx->gens_comp.p + (size_t)row * 8, 32, hipMemcpyDeviceToHost));
    return DAPOL_OK;
}

// ------------------------------------------------------------------------------------------- commitments
int32_t dapol_commit_hash_batch(dapol_ctx* ctx, size_t n, const uint64_t* v, const uint8_t* r32, uint8_t* C_out32, uint8_t* H_out32) {
    if (!ctx || (n && (!v || !r32 || !C_out32 || !H_out32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf<uint64_t> dv;
    DevBuf<uint32_t> dr, dC, dH, dHw;
    HIPCHK(dv.alloc(n)); HIPCHK(dr.alloc(n * 8)); HIPCHK(dC.alloc(n * 8)); HIPCHK(dH.alloc(n * 8));
    HIPCHK(hipMemcpyAsync(dv.p, v, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dr.p, r32, n * 32, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH_DX(ctx->tv.digest, (k_commit_hash<DX>), dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, ctx->tv, n, dv.p, dr.p, dC.p, dH.p, (int32_t*)nullptr);
    LAUNCH_CHECK();
    if (ctx_wide(ctx)) {                           // 64-byte digest: H = D(C) over the commitments just made
        HIPCHK(dHw.alloc(n * 16));
        hipLaunchKernelGGL(k_wide_hash_leaves, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, n, dC.p, dHw.p);
        LAUNCH_CHECK();
    }
    HIPCHK(hipMemcpyAsync(C_out32, dC.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(H_out32, ctx_wide(ctx) ? dHw.p : dH.p, n * ctx_hash_bytes(ctx), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DAPOL_OK;
}

#include "host_tree.inc"
#include "host_tree_edit.inc"
#include "host_range.inc"
#include "host_policy.inc"
#include "host_entity.inc"
#include "host_workload.inc"
#include "host_shared.inc"
#include "host_reprove.inc"
#include "host_verify.inc"
#include "host_verify_shared.inc"
#include "host_verify_compact.inc"
#include "host_compact_paths.inc"
#include "host_store.inc"
#include "host_leaf.inc"
#include "host_wire.inc"
#include "host_batch.inc"
#include "host_batches.inc"
#include "host_reprove_batches.inc"
#include "host_batch_store.inc"
#include "host_comm.inc"
