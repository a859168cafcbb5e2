// dapol_reprove_batches / dapol_reprove_batches_plan as index arithmetic: which edited leaves lie below a sibling of a batch, which
// (batch, sub-proof) pairs an edit therefore makes DIRTY, the first nonce slot of every sub-proof of a plan, and where the dirty
// pairs of each m-CLASS (all dirty sub-proofs of one m, whatever their batch's sibling count) lie in the compact buffers.  Pure
// functions, no HIP call and no context: the kernels (kernels_reprove_batches.h) and the host side (host_reprove_batches.inc) call
// them, and tests/cpp/reprove_batches_plan_host.cpp replays them on the CPU under ASan + UBSan
// (tests/test_reprove_batches_host_asan.py).  The includer provides the DAPOL_POLICY_* constants.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "policy_plan.inc"

#if defined(__HIPCC__)
#define RBP_HD __host__ __device__ __forceinline__
#else
#define RBP_HD inline
#endif

// Does an edited leaf lie below the node (level, index)?  level 0 = leaves, at most 63 (a sibling is never the root); the node covers
// the leaves index << level .. that | (2^level - 1).  One binary search over the strictly increasing edits: the first edit >= lo.
static inline bool reprove_batches_below(int level, uint64_t index, size_t k, const uint64_t* edited) {
    const unsigned sh = (unsigned)level;                         // 0 .. 63
    const uint64_t lo = index << sh, hi = lo | ((1ull << sh) - 1);
    size_t a = 0, z = k;
    while (a < z) { const size_t mid = a + (z - a) / 2; if (edited[mid] < lo) a = mid + 1; else z = mid; }
    return a < k && edited[a] <= hi;
}

static inline bool reprove_batches_increasing_below(int H, size_t n, const uint64_t* idx) {
    for (size_t i = 1; i < n; i++) if (idx[i] <= idx[i - 1]) return false;
    return !(n && H < 64 && (idx[n - 1] >> H) != 0);
}

// One batch of the plan call: `sibs` are the batch's S sibling positions in proof order (anything with .level and .index), `plan` the
// policy's plan over S.  Returns the batch's dirty sub-proofs and adds to the sums.  A batch's own leaves lie below none of its
// siblings, so an edit of one of them dirties nothing here.
struct ReproveBatchesPlanOut { uint64_t total_proved = 0, sum_m_proved = 0, sum_m_all = 0; };
template <typename Sib>
static inline uint64_t reprove_batches_plan_batch(const std::vector<SubProof>& plan, const Sib* sibs, bool has_old, size_t k, const uint64_t* edited,
                                                  ReproveBatchesPlanOut& out) {
    uint64_t proved = 0;
    for (const SubProof& sp : plan) {
        bool dirty = !has_old;
        for (int i = sp.start; !dirty && i < sp.start + sp.count; i++) dirty = reprove_batches_below(sibs[i].level, sibs[i].index, k, edited);
        out.sum_m_all += (uint64_t)sp.m;
        if (dirty) { proved++; out.sum_m_proved += (uint64_t)sp.m; }
    }
    out.total_proved += proved;
    return proved;
}

// One sub-proof of one distinct plan of a call, as the kernels read it: which siblings, which class, the first nonce slot inside the
// batch's draws (policy_layout's running sum: every earlier sub-proof of the plan takes m (2 n_bits + 4) slots, grouped or not) and
// its 16-byte pieces inside the batch's blob.
struct ReproveBatchesEntry {
    uint32_t start, count, m, cls;
    uint64_t slot;
    uint32_t piece0, pieces;
};
static inline void reprove_batches_entries(const std::vector<SubProof>& plan, int n_bits, const std::vector<uint32_t>& class_m,
                                           std::vector<ReproveBatchesEntry>& tab) {
    uint64_t slot = 0;
    uint32_t piece = 0;
    for (const SubProof& sp : plan) {
        uint32_t cls = 0;
        while (cls < class_m.size() && class_m[cls] != (uint32_t)sp.m) cls++;
        const uint32_t pieces = (uint32_t)(dapol_range_proof_size(n_bits, sp.m) / 16);
        tab.push_back({(uint32_t)sp.start, (uint32_t)sp.count, (uint32_t)sp.m, cls, slot, piece, pieces});
        slot += (uint64_t)sp.m * (2 * (uint64_t)n_bits + 4);
        piece += pieces;
    }
}

// The flags are class-major: flag[cls][pair] over all n pairs of the call, then one closing zero.  After the inclusive scan a dirty
// pair of class cls has the compact row rank - 1 over the whole call (classes in ascending m) and rank - 1 - before[cls] in its class.
enum { REPROVE_BATCHES_MAX_CLASSES = 24 };                   // m is a power of two <= 2^20 (batches_shape)
RBP_HD size_t reprove_batches_flag_at(uint32_t cls, size_t n_pairs, size_t pair) { return (size_t)cls * n_pairs + pair; }
// The element of the scan that holds the dirty pairs before class cls; SIZE_MAX: none before it.
static inline size_t reprove_batches_base_at(uint32_t cls, size_t n_pairs) { return cls == 0 ? (size_t)-1 : (size_t)cls * n_pairs - 1; }

struct ReproveBatchesClasses {
    uint32_t n;                                              // classes of the call
    uint32_t m[REPROVE_BATCHES_MAX_CLASSES];
    uint32_t pieces[REPROVE_BATCHES_MAX_CLASSES];            // 16-byte pieces of one proof of the class
    uint32_t before[REPROVE_BATCHES_MAX_CLASSES + 1];        // dirty pairs before the class; [n]: all of them
    uint64_t party_off[REPROVE_BATCHES_MAX_CLASSES];         // the class's parties in the compact [U][m] arrays
    uint64_t piece_off[REPROVE_BATCHES_MAX_CLASSES];         // its proofs in the compact proof buffer (16-byte pieces)
    uint64_t parties, proof_pieces;                          // totals
};
// before[0 .. n] filled in: the places of the classes' rows.
static inline void reprove_batches_layout(ReproveBatchesClasses& K) {
    K.parties = 0; K.proof_pieces = 0;
    for (uint32_t c = 0; c < K.n; c++) {
        const uint64_t U = (uint64_t)K.before[c + 1] - (uint64_t)K.before[c];
        K.party_off[c] = K.parties; K.piece_off[c] = K.proof_pieces;
        K.parties += U * K.m[c]; K.proof_pieces += U * K.pieces[c];
    }
}
