// Multi-GPU exchange step of the sharded path (SURVEY.md section 8e) as RCCL call sites inside the library, so that a host in
// any language gets it through the C ABI: ONE ncclAllGather of the G subtree-root records (104 bytes each, latency-bound
// over xGMI), the replicated merge of the top log2 G levels on every rank's own GPU, and ncclAllReduce for the final
// reduce of the proof checksums / verdict counts.  The reference has no communication at all (single process, single
// thread); there is nothing to translate.  Included from dapol_hip.hip, last.
#include <rccl/rccl.h>
#include <chrono>
#include <thread>

struct dapol_comm {
    dapol_ctx* ctx = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, shard_bits = 0;
    bool holds_ctx = false;
    long long coll_timeout_ms = -1;      // deadline of every collective (enqueue + completion); < 0: none
    hipEvent_t ev = nullptr;             // marks the end of a collective on the context's stream
    hipEvent_t tev[3] = {nullptr, nullptr, nullptr};   // timing: before the collective, after it, after the replicated top levels
    dapol_comm_timing tm = {};           // dapol_comm_timing_get
    DevBuf<uint8_t> send, recv;          // 104-byte record, world records
    DevBuf<uint64_t> red;
};

static int32_t fail_nccl(ncclResult_t r, const char* what, int line) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s failed at host_comm.inc:%d: %s", what, line, ncclGetErrorString(r));
    g_last_error = buf;
    return DAPOL_ERR_COMM;
}
#define NCCLCHK(x)                                                    \
    do {                                                              \
        ncclResult_t r_ = (x);                                        \
        if (r_ != ncclSuccess) return fail_nccl(r_, #x, __LINE__);    \
    } while (0)

int32_t dapol_comm_unique_id(uint8_t id_out[DAPOL_COMM_ID_BYTES]) {
    if (!id_out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    static_assert(sizeof(ncclUniqueId) == DAPOL_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return DAPOL_OK;
}

// RCCL calls on a NON-BLOCKING communicator return ncclInProgress while the work is still being set up; this polls the
// communicator's state until it settles or the deadline passes (deadline_ms < 0: no deadline).
static ncclResult_t nccl_settle(ncclComm_t comm, ncclResult_t r, long long deadline_ms) {
    if (r != ncclInProgress) return r;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        ncclResult_t st = ncclSuccess;
        ncclResult_t q = ncclCommGetAsyncError(comm, &st);
        if (q != ncclSuccess) return q;
        if (st != ncclInProgress) return st;
        if (deadline_ms >= 0 && std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > deadline_ms)
            return ncclInProgress;
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
}
// A collective that cannot finish must not hang the caller for good (a peer that died, a transport that came up and then broke).
// A communicator created with a deadline (dapol_comm_create_timeout) keeps one for its collectives: if the call does not settle,
// or what it put on the stream has not completed, by then -- or RCCL reports an asynchronous error meanwhile -- the communicator
// is ABORTED here (ncclCommAbort is what ends an RCCL kernel that waits for a peer; the stream then drains), every later call on
// it fails at once, and the caller gets DAPOL_ERR_COMM: the host falls back to another transport or exits.
static int32_t comm_fail(dapol_comm* c, ncclResult_t r, const char* what, int line) {
    if (c->comm) { (void)ncclCommAbort(c->comm); c->comm = nullptr; }
    if (r == ncclInProgress) {
        char buf[200];
        snprintf(buf, sizeof buf, "%s did not complete within %lld ms (rank %d of %d): communicator aborted (host_comm.inc:%d)", what, c->coll_timeout_ms, c->rank, c->world, line);
        g_last_error = buf;
        return DAPOL_ERR_COMM;
    }
    return fail_nccl(r, what, line);
}
#define NCCLCHK_COMM(c, x)                                                                  \
    do {                                                                                    \
        if (!(c)->comm) return fail(DAPOL_ERR_COMM, "the communicator was aborted");        \
        ncclResult_t r_ = nccl_settle((c)->comm, (x), (c)->coll_timeout_ms);                \
        if (r_ != ncclSuccess) return comm_fail((c), r_, #x, __LINE__);                     \
    } while (0)
// Waits for what has been put on `st` so far (the collective and the copies around it), with the communicator's deadline.
static int32_t comm_wait(dapol_comm* c, hipStream_t st, const char* what, int line) {
    if (c->coll_timeout_ms < 0) { HIPCHK(hipStreamSynchronize(st)); return DAPOL_OK; }
    HIPCHK(hipEventRecord(c->ev, st));
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; spins++) {
        hipError_t e = hipEventQuery(c->ev);
        if (e == hipSuccess) return DAPOL_OK;
        if (e != hipErrorNotReady) return fail_hip(e, what, "host_comm.inc", line);
        (void)hipGetLastError();
        const long long ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        if ((spins & 63) == 63 || ms > 5) {
            ncclResult_t as = ncclSuccess;
            ncclResult_t q = ncclCommGetAsyncError(c->comm, &as);
            if (q != ncclSuccess) return comm_fail(c, q, what, line);
            if (as != ncclSuccess && as != ncclInProgress) return comm_fail(c, as, what, line);
            if (ms > c->coll_timeout_ms) {
                int32_t rc = comm_fail(c, ncclInProgress, what, line);
                (void)hipStreamSynchronize(st);                      // (the aborted kernel leaves; nothing of this call stays queued)
                return rc;
            }
        }
        if (ms > 5) std::this_thread::sleep_for(std::chrono::microseconds(200));
        else std::this_thread::yield();
    }
}

// ncclCommInitRank blocks until every rank has called it, and a rank that never arrives would hang the others for good.  The
// communicator is therefore created non-blocking (ncclCommInitRankConfig, blocking = 0) and polled (ncclCommGetAsyncError) up to
// a deadline; a communicator that has not come up by then is ABORTED (ncclCommAbort), not abandoned, and the call returns
// DAPOL_ERR_COMM -- the host can then fall back to another transport or exit.  timeout_ms <= 0: wait without a deadline.
int32_t dapol_comm_create_timeout(dapol_ctx* ctx, const uint8_t id[DAPOL_COMM_ID_BYTES], int32_t rank, int32_t world, int64_t timeout_ms, dapol_comm** out) {
    if (!ctx || !id || !out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    NEEDS_32_BYTE_DIGEST(ctx, "the sharded (multi-GPU) path");       // (its records are 104 bytes: C | H32 | v | r)
    if (world < 1 || world > 65536 || (world & (world - 1)) || rank < 0 || rank >= world)
        return fail(DAPOL_ERR_INVALID_ARGUMENT, "world must be a power of two (each rank owns one top-level subtree) and 0 <= rank < world");
    HIPCHK(hipSetDevice(ctx->device));
    dapol_comm* c = new dapol_comm();
    struct Guard { dapol_comm* c; ~Guard() { if (c) dapol_comm_abort(c); } } guard{c};
    c->ctx = ctx; c->rank = rank; c->world = world;
    while ((1 << c->shard_bits) < world) c->shard_bits++;
    HIPCHK(c->send.alloc(DAPOL_RECORD_BYTES)); HIPCHK(c->recv.alloc((size_t)world * DAPOL_RECORD_BYTES)); HIPCHK(c->red.alloc(64));
    HIPCHK(hipEventCreateWithFlags(&c->ev, hipEventDisableTiming));
    for (auto& e : c->tev) HIPCHK(hipEventCreate(&e));
    c->coll_timeout_ms = timeout_ms > 0 ? (long long)timeout_ms : -1;
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    ncclResult_t r = ncclCommInitRankConfig(&c->comm, world, uid, rank, &cfg);
    if (r != ncclSuccess && r != ncclInProgress) { c->comm = nullptr; return fail_nccl(r, "ncclCommInitRankConfig", __LINE__); }
    r = nccl_settle(c->comm, ncclInProgress, timeout_ms > 0 ? (long long)timeout_ms : -1);
    if (r == ncclInProgress) {
        char buf[160];
        snprintf(buf, sizeof buf, "the RCCL communicator did not come up within %lld ms (rank %d of %d): aborted", (long long)timeout_ms, rank, world);
        g_last_error = buf;
        return DAPOL_ERR_COMM;                       // (the guard aborts the half-made communicator)
    }
    if (r != ncclSuccess) return fail_nccl(r, "ncclCommInitRankConfig (async)", __LINE__);
    ctx_retain(ctx);
    c->holds_ctx = true;
    guard.c = nullptr;
    *out = c;
    return DAPOL_OK;
}
int32_t dapol_comm_create(dapol_ctx* ctx, const uint8_t id[DAPOL_COMM_ID_BYTES], int32_t rank, int32_t world, dapol_comm** out) {
    return dapol_comm_create_timeout(ctx, id, rank, world, 0, out);
}

static int32_t comm_release(dapol_comm* c, bool abort) {
    if (!c) return DAPOL_OK;
    dapol_ctx* ctx = c->holds_ctx ? c->ctx : nullptr;       // a fully created communicator holds a context reference
    if (c->ctx) (void)hipSetDevice(c->ctx->device);
    if (c->comm) {
        if (abort) (void)ncclCommAbort(c->comm);
        else {
            // a non-blocking communicator is finalised first (flushes what was issued), then destroyed
            ncclResult_t r = nccl_settle(c->comm, ncclCommFinalize(c->comm), 10000);
            if (r == ncclSuccess) (void)ncclCommDestroy(c->comm);
            else (void)ncclCommAbort(c->comm);
        }
    }
    if (c->ev) (void)hipEventDestroy(c->ev);
    for (auto e : c->tev) if (e) (void)hipEventDestroy(e);
    delete c;
    if (ctx) (void)dapol_ctx_destroy(ctx);
    return DAPOL_OK;
}
int32_t dapol_comm_destroy(dapol_comm* c) { return comm_release(c, false); }
// The failure path: tears the communicator down without waiting for the peers (ncclCommAbort).  Use it when the ranks have
// agreed that the exchange will not go through this communicator (one of them failed to create its own).
int32_t dapol_comm_abort(dapol_comm* c) { return comm_release(c, true); }
// Ranks the communicator spans as RCCL itself reports it (ncclCommCount) -- the bench prints it next to the exchange path.
int32_t dapol_comm_count(dapol_comm* c, int32_t* count) {
    if (!c || !count) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (!c->comm) return fail(DAPOL_ERR_COMM, "the communicator was aborted");
    int n = 0;
    NCCLCHK(ncclCommCount(c->comm, &n));
    *count = n;
    return DAPOL_OK;
}

// parents of n pairs of records: out[i] = merge(in[2i], in[2i+1])  (Mergeable::merge, src/dapol/node.rs:64-80)
template <int DX>
__global__ void k_merge_pairs(int dg, size_t n, const uint32_t* C, const uint32_t* H, const uint64_t* v, const uint32_t* r, uint32_t* oC, uint32_t* oH,
                              uint64_t* ov, uint32_t* orr, uint32_t* bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t cl[8], cr[8], hl[8], hr[8], cp[8], hp[8], ra[8], rb[8], rp[8];
    ld8(cl, C + 16 * i); ld8(cr, C + 16 * i + 8); ld8(hl, H + 16 * i); ld8(hr, H + 16 * i + 8);
    ge_p3 a, b, p;
    if (!(ge_decompress(a, cl) & ge_decompress(b, cr))) { atomicOr(bad, 1u); return; }
    ge_add(p, a, b);
    ge_compress(cp, p);
    node_hash128_x<DX>(dg, hp, cl, cr, hl, hr);
    ld8(ra, r + 16 * i); ld8(rb, r + 16 * i + 8);
    sc ma, mb, ms;
    sc_to_mont(ma, ra); sc_to_mont(mb, rb); sc_add(ms, ma, mb); sc_from_mont(rp, ms);
    st8(oC + 8 * i, cp); st8(oH + 8 * i, hp); st8(orr + 8 * i, rp);
    ov[i] = v[2 * i] + v[2 * i + 1];
}
// records [g][104] (C | H | v LE64 | r) -> SoA
__global__ void k_unpack_records(size_t g, const uint8_t* rec, uint32_t* C, uint32_t* H, uint64_t* v, uint32_t* r) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g) return;
    const uint8_t* p = rec + i * DAPOL_RECORD_BYTES;
    auto word = [&](int off) { return (uint32_t)p[off] | ((uint32_t)p[off + 1] << 8) | ((uint32_t)p[off + 2] << 16) | ((uint32_t)p[off + 3] << 24); };
    for (int k = 0; k < 8; k++) { C[8 * i + k] = word(4 * k); H[8 * i + k] = word(32 + 4 * k); r[8 * i + k] = word(72 + 4 * k); }
    v[i] = (uint64_t)word(64) | ((uint64_t)word(68) << 32);
}

// The replicated top of the tree from the G subtree-root records already on this GPU: root record and the log2 G
// siblings above `rank`'s subtree root, root side first.  Also used with records a caller gathered by other means.
static int32_t top_levels_device(dapol_ctx* ctx, int world, int rank, const uint8_t* d_records, uint8_t root_C[32], uint8_t root_H[32],
                                 uint64_t* root_v, uint8_t root_r[32], uint8_t* up_C32, uint8_t* up_H32, uint64_t* up_v, uint8_t* up_r32) {
    hipStream_t st = ctx->stream;
    int bits = 0;
    while ((1 << bits) < world) bits++;
    const size_t G = (size_t)world;
    DevBuf<uint32_t> C[2], H[2], r[2], bad;
    DevBuf<uint64_t> v[2];
    for (int i = 0; i < 2; i++) { HIPCHK(C[i].alloc(G * 8)); HIPCHK(H[i].alloc(G * 8)); HIPCHK(r[i].alloc(G * 8)); HIPCHK(v[i].alloc(G)); }
    HIPCHK(bad.alloc(1));
    HIPCHK(hipMemsetAsync(bad.p, 0, 4, st));
    hipLaunchKernelGGL(k_unpack_records, dim3(nblk(G, 64)), dim3(64), 0, st, G, d_records, C[0].p, H[0].p, v[0].p, r[0].p);
    LAUNCH_CHECK();
    int cur = 0, pos = rank;
    size_t g = G;
    for (int lvl = 0; lvl < bits; lvl++) {
        const size_t s = (size_t)(pos ^ 1);
        const int slot = bits - 1 - lvl;                       // root side first
        if (up_C32) HIPCHK(hipMemcpyAsync(up_C32 + 32 * slot, C[cur].p + 8 * s, 32, hipMemcpyDeviceToHost, st));
        if (up_H32) HIPCHK(hipMemcpyAsync(up_H32 + 32 * slot, H[cur].p + 8 * s, 32, hipMemcpyDeviceToHost, st));
        if (up_r32) HIPCHK(hipMemcpyAsync(up_r32 + 32 * slot, r[cur].p + 8 * s, 32, hipMemcpyDeviceToHost, st));
        if (up_v) HIPCHK(hipMemcpyAsync(up_v + slot, v[cur].p + s, 8, hipMemcpyDeviceToHost, st));
        LAUNCH_DX(ctx->tv.digest, (k_merge_pairs<DX>), dim3(nblk(g / 2, 64)), dim3(64), 0, st, ctx->tv.digest, g / 2, C[cur].p, H[cur].p, v[cur].p, r[cur].p,
                           C[cur ^ 1].p, H[cur ^ 1].p, v[cur ^ 1].p, r[cur ^ 1].p, bad.p);
        LAUNCH_CHECK();
        cur ^= 1; g /= 2; pos >>= 1;
    }
    uint32_t h_bad = 0;
    HIPCHK(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    if (root_C) HIPCHK(hipMemcpyAsync(root_C, C[cur].p, 32, hipMemcpyDeviceToHost, st));
    if (root_H) HIPCHK(hipMemcpyAsync(root_H, H[cur].p, 32, hipMemcpyDeviceToHost, st));
    if (root_r) HIPCHK(hipMemcpyAsync(root_r, r[cur].p, 32, hipMemcpyDeviceToHost, st));
    if (root_v) HIPCHK(hipMemcpyAsync(root_v, v[cur].p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_bad) return fail(DAPOL_ERR_VALUE_DECODING, "a subtree-root commitment does not decode");
    return DAPOL_OK;
}

static void pack_record(uint8_t* rec, const uint8_t C[32], const uint8_t H[32], uint64_t v, const uint8_t r[32]) {
    memcpy(rec, C, 32); memcpy(rec + 32, H, 32);
    for (int i = 0; i < 8; i++) rec[64 + i] = (uint8_t)(v >> (8 * i));
    memcpy(rec + 72, r, 32);
}

int32_t dapol_shard_exchange(dapol_comm* c, const uint8_t sub_C[32], const uint8_t sub_H[32], uint64_t sub_v, const uint8_t sub_r[32],
                             uint8_t root_C[32], uint8_t root_H[32], uint64_t* root_v, uint8_t root_r[32], uint8_t* up_C32, uint8_t* up_H32,
                             uint64_t* up_v, uint8_t* up_r32, uint8_t* records_out) {
    if (!c || !sub_C || !sub_H || !sub_r) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    dapol_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const auto h0 = std::chrono::steady_clock::now();
    uint8_t rec[DAPOL_RECORD_BYTES];
    pack_record(rec, sub_C, sub_H, sub_v, sub_r);
    HIPCHK(hipMemcpyAsync(c->send.p, rec, DAPOL_RECORD_BYTES, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->tev[0], st));
    NCCLCHK_COMM(c, ncclAllGather(c->send.p, c->recv.p, DAPOL_RECORD_BYTES, ncclUint8, c->comm, st));     // the one layer-boundary exchange
    HIPCHK(hipEventRecord(c->tev[1], st));
    { int32_t rc = comm_wait(c, st, "ncclAllGather", __LINE__); if (rc) return rc; }
    if (records_out) HIPCHK(hipMemcpyAsync(records_out, c->recv.p, (size_t)c->world * DAPOL_RECORD_BYTES, hipMemcpyDeviceToHost, st));
    int32_t rc = top_levels_device(ctx, c->world, c->rank, c->recv.p, root_C, root_H, root_v, root_r, up_C32, up_H32, up_v, up_r32);
    if (rc) return rc;
    // timing of THIS call (device time of the all-gather incl. the wait for the slowest peer, the replicated top levels incl. their
    // copies back, the whole call on the host clock): the bench's N > 1 lines carry them per step
    HIPCHK(hipEventRecord(c->tev[2], st));
    HIPCHK(hipEventSynchronize(c->tev[2]));
    float ag_ms = 0.f, top_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ag_ms, c->tev[0], c->tev[1]));
    HIPCHK(hipEventElapsedTime(&top_ms, c->tev[1], c->tev[2]));
    dapol_comm_timing& tm = c->tm;
    tm.exchanges++;
    tm.last_allgather_us = 1e3 * ag_ms; tm.last_top_levels_us = 1e3 * top_ms;
    tm.last_exchange_host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count();
    tm.sum_allgather_us += tm.last_allgather_us; tm.sum_top_levels_us += tm.last_top_levels_us; tm.sum_exchange_host_us += tm.last_exchange_host_us;
    return DAPOL_OK;
}

int32_t dapol_shard_top_levels(dapol_ctx* ctx, int32_t world, int32_t rank, const uint8_t* records, uint8_t root_C[32], uint8_t root_H[32],
                               uint64_t* root_v, uint8_t root_r[32], uint8_t* up_C32, uint8_t* up_H32, uint64_t* up_v, uint8_t* up_r32) {
    if (!ctx || !records) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    NEEDS_32_BYTE_DIGEST(ctx, "the sharded (multi-GPU) path");
    if (world < 1 || world > 65536 || (world & (world - 1)) || rank < 0 || rank >= world) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad world / rank");
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf<uint8_t> d;
    HIPCHK(d.alloc((size_t)world * DAPOL_RECORD_BYTES));
    HIPCHK(hipMemcpyAsync(d.p, records, (size_t)world * DAPOL_RECORD_BYTES, hipMemcpyHostToDevice, ctx->stream));
    return top_levels_device(ctx, world, rank, d.p, root_C, root_H, root_v, root_r, up_C32, up_H32, up_v, up_r32);
}

int32_t dapol_comm_allreduce_u64(dapol_comm* c, int32_t op, uint64_t* inout, size_t n) {
    if (!c || (n && !inout)) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    if (n > 64) return fail(DAPOL_ERR_INVALID_ARGUMENT, "at most 64 words per reduce (checksums, counts, verdict masks)");
    if (op != DAPOL_REDUCE_SUM && op != DAPOL_REDUCE_MIN && op != DAPOL_REDUCE_MAX) return fail(DAPOL_ERR_INVALID_ARGUMENT, "bad reduce op");
    if (n == 0) return DAPOL_OK;
    dapol_ctx* ctx = c->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const auto h0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(c->red.p, inout, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->tev[0], st));
    ncclRedOp_t rop = op == DAPOL_REDUCE_SUM ? ncclSum : (op == DAPOL_REDUCE_MIN ? ncclMin : ncclMax);
    NCCLCHK_COMM(c, ncclAllReduce(c->red.p, c->red.p, n, ncclUint64, rop, c->comm, st));                   // wrapping 64-bit sum: the final reduce
    // Wait FIRST, with the deadline, and copy back only on success (as dapol_shard_exchange does): a device-to-host copy into the
    // caller's pageable memory blocks the host until the stream drains -- queued behind an all-reduce whose peer is dead it would
    // hang inside hipMemcpyAsync, before the deadline and ncclCommAbort below were ever reached.
    HIPCHK(hipEventRecord(c->tev[1], st));
    { int32_t rc = comm_wait(c, st, "ncclAllReduce", __LINE__); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(inout, c->red.p, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ar_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ar_ms, c->tev[0], c->tev[1]));
    dapol_comm_timing& tm = c->tm;
    tm.reduces++;
    tm.last_allreduce_us = 1e3 * ar_ms;
    tm.last_reduce_host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count();
    tm.sum_allreduce_us += tm.last_allreduce_us; tm.sum_reduce_host_us += tm.last_reduce_host_us;
    return DAPOL_OK;
}

int32_t dapol_comm_timing_get(dapol_comm* c, dapol_comm_timing* out, int32_t reset) {
    if (!c || !out) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    *out = c->tm;
    if (reset) c->tm = dapol_comm_timing{};
    return DAPOL_OK;
}

// Any node of the replicated top of a sharded tree, from the G subtree-root records: level_above = 0 (the shard roots) ..
// log2 G (the global root), index within that level.  Batched proofs need these for the siblings above the shard roots.
int32_t dapol_shard_top_node_records(dapol_ctx* ctx, int32_t world, const uint8_t* records, size_t n, const uint8_t* level_above, const uint64_t* index,
                                     uint8_t* C32, uint8_t* H32, uint64_t* v, uint8_t* r32) {
    if (!ctx || !records || (n && (!level_above || !index || !C32 || !H32 || !v || !r32))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "null argument");
    NEEDS_32_BYTE_DIGEST(ctx, "the sharded (multi-GPU) path");
    if (world < 1 || world > 65536 || (world & (world - 1))) return fail(DAPOL_ERR_INVALID_ARGUMENT, "world must be a power of two");
    int bits = 0;
    while ((1 << bits) < world) bits++;
    for (size_t i = 0; i < n; i++)
        if (level_above[i] > bits || index[i] >= ((uint64_t)world >> level_above[i])) return fail(DAPOL_ERR_INVALID_ARGUMENT, "node outside the top of the tree");
    if (n == 0) return DAPOL_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t G = (size_t)world;
    // all levels of the top, concatenated: level t starts at off[t], G >> t nodes
    std::vector<size_t> off((size_t)bits + 2, 0);
    for (int t = 0; t <= bits; t++) off[t + 1] = off[t] + (G >> t);
    const size_t tot = off[bits + 1];
    DevBuf<uint8_t> drec;
    DevBuf<uint32_t> C, H, r, bad;
    DevBuf<uint64_t> vv;
    HIPCHK(drec.alloc(G * DAPOL_RECORD_BYTES)); HIPCHK(C.alloc(tot * 8)); HIPCHK(H.alloc(tot * 8)); HIPCHK(r.alloc(tot * 8)); HIPCHK(vv.alloc(tot)); HIPCHK(bad.alloc(1));
    HIPCHK(hipMemsetAsync(bad.p, 0, 4, st));
    HIPCHK(hipMemcpyAsync(drec.p, records, G * DAPOL_RECORD_BYTES, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_unpack_records, dim3(nblk(G, 64)), dim3(64), 0, st, G, drec.p, C.p, H.p, vv.p, r.p);
    LAUNCH_CHECK();
    for (int t = 0; t < bits; t++) {
        const size_t g = G >> t, a = off[t], b = off[t + 1];
        LAUNCH_DX(ctx->tv.digest, (k_merge_pairs<DX>), dim3(nblk(g / 2, 64)), dim3(64), 0, st, ctx->tv.digest, g / 2, C.p + a * 8, H.p + a * 8, vv.p + a, r.p + a * 8,
                           C.p + b * 8, H.p + b * 8, vv.p + b, r.p + b * 8, bad.p);
        LAUNCH_CHECK();
    }
    uint32_t h_bad = 0;
    HIPCHK(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, st));
    for (size_t i = 0; i < n; i++) {
        const size_t s = off[level_above[i]] + (size_t)index[i];
        HIPCHK(hipMemcpyAsync(C32 + 32 * i, C.p + s * 8, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(H32 + 32 * i, H.p + s * 8, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(r32 + 32 * i, r.p + s * 8, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(v + i, vv.p + s, 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (h_bad) return fail(DAPOL_ERR_VALUE_DECODING, "a subtree-root commitment does not decode");
    return DAPOL_OK;
}
