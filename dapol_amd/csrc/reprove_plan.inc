// dapol_reprove_entities_shared / dapol_reprove_plan as index arithmetic: the key shift of a sub-proof, the depths its siblings occupy,
// which (sub-proof, row) pairs an edit of the tree makes DIRTY and which of them are HEADS, the way from a rank to a compact row when
// row 0 of a group need not be a head, and where the groups' head rows lie in the compact buffers.  Pure functions, no HIP call and no
// context: the kernels (kernels_reprove.h) and the host side (host_reprove.inc) call them, and tests/cpp/reprove_plan_asan.cpp replays
// them on the CPU under ASan + UBSan (tests/test_reprove_plan_cpu.py).  The includer provides the DAPOL_POLICY_* constants.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "policy_plan.inc"

#if defined(__HIPCC__)
#define RPP_HD __host__ __device__ __forceinline__
#else
#define RPP_HD inline
#endif

// H - D of a sub-proof (D = its key depth, include/dapol_hip.h; 64: the key is 0 -- never used as a shift count)
static inline unsigned reprove_shift(const SubProof& sp, int H, bool leaf_first) {
    const int D = sp.count == 0 ? 0 : leaf_first ? H - sp.start : sp.start + sp.count;
    return (unsigned)(H - D);
}
static inline uint64_t reprove_key(uint64_t idx, unsigned shift) { return shift >= 64 ? 0ull : (idx >> shift) << shift; }
// Bit d - 1 set for every depth d (1 .. H below the root) that one of the sub-proof's siblings occupies.
static inline uint64_t reprove_depth_mask(const SubProof& sp, int H, bool leaf_first) {
    uint64_t m = 0;
    for (int i = sp.start; i < sp.start + sp.count; i++) m |= 1ull << ((leaf_first ? H - i : i + 1) - 1);
    return m;
}
// Bit d - 1 set where the sibling of `leaf` at depth d holds an edited leaf: the sibling is the depth-d node whose index is the leaf's
// prefix with its last bit flipped, and it covers the leaves lo .. lo | (2^(H - d) - 1).  Two binary searches per depth over the
// strictly increasing edits; the leaf's own edit lies under none of its siblings.
static inline uint64_t reprove_dirty_depths(uint64_t leaf, int H, size_t k, const uint64_t* edited) {
    uint64_t mask = 0;
    for (int d = 1; d <= H && k; d++) {
        const unsigned sh = (unsigned)(H - d);                   // 0 .. 63
        const uint64_t lo = ((leaf >> sh) ^ 1ull) << sh, hi = lo | ((1ull << sh) - 1);
        size_t a = 0, z = k;                                     // first edit >= lo
        while (a < z) { const size_t mid = a + (z - a) / 2; if (edited[mid] < lo) a = mid + 1; else z = mid; }
        size_t c = a, y = k;                                     // first edit > hi
        while (c < y) { const size_t mid = c + (y - c) / 2; if (edited[mid] <= hi) c = mid + 1; else y = mid; }
        if (c > a) mask |= 1ull << (d - 1);
    }
    return mask;
}

static inline bool reprove_increasing_below(int H, size_t n, const uint64_t* idx) {
    for (size_t i = 1; i < n; i++) if (idx[i] <= idx[i - 1]) return false;
    return !(n && H < 64 && (idx[n - 1] >> H) != 0);
}

// The planner: heads per sub-proof and the sums.  false: bad indexes (the plan is the caller's, already made).
struct ReprovePlanOut { uint64_t total_proved = 0, sum_m_proved = 0, sum_m_shared = 0; };
static bool reprove_plan_host(const std::vector<SubProof>& plan, int H, bool leaf_first, size_t b, const uint64_t* leaf_idx, const uint8_t* has_old, size_t k,
                              const uint64_t* edited, uint64_t* n_proved_out, ReprovePlanOut& out) {
    out = ReprovePlanOut{};
    if (!reprove_increasing_below(H, b, leaf_idx) || !reprove_increasing_below(H, k, edited)) return false;
    const size_t ns = plan.size();
    std::vector<uint64_t> smask(ns), heads(ns, 0), uniq(ns, 0);
    std::vector<unsigned> shift(ns);
    std::vector<uint8_t> prev_dirty(ns, 0);
    for (size_t s = 0; s < ns; s++) { smask[s] = reprove_depth_mask(plan[s], H, leaf_first); shift[s] = reprove_shift(plan[s], H, leaf_first); }
    for (size_t e = 0; e < b; e++) {
        const bool old = !has_old || has_old[e];
        const uint64_t depths = old ? reprove_dirty_depths(leaf_idx[e], H, k, edited) : 0;
        for (size_t s = 0; s < ns; s++) {
            const bool new_key = e == 0 || reprove_key(leaf_idx[e], shift[s]) != reprove_key(leaf_idx[e - 1], shift[s]);
            const bool dirty = !old || (depths & smask[s]) != 0;
            if (dirty && (new_key || !prev_dirty[s])) heads[s]++;
            if (new_key) uniq[s]++;
            prev_dirty[s] = dirty ? 1 : 0;
        }
    }
    for (size_t s = 0; s < ns; s++) {
        if (n_proved_out) n_proved_out[s] = heads[s];
        out.total_proved += heads[s];
        out.sum_m_proved += heads[s] * (uint64_t)plan[s].m;
        out.sum_m_shared += uniq[s] * (uint64_t)plan[s].m;
    }
    return true;
}

// rank = the inclusive scan of the head flags in plan order (s-major).  A dirty (s, e) -- a head, or a row of a head's run -- has the
// compact row rank[s][e] - 1 over the whole call and rank[s][e] - 1 - (heads before the group) inside its group.  Row 0 of a group
// may be kept, so the group's base is NOT rank[s0][0] - 1: it is the scan's element before (s0, 0), 0 for the first group.
RPP_HD size_t reprove_group_row(uint32_t rank_f, uint32_t heads_before_group) { return (size_t)rank_f - 1 - (size_t)heads_before_group; }
// The element of the scan that holds the heads before group gi (whose first sub-proof is s0); SIZE_MAX: none before it.
static inline size_t reprove_base_at(uint32_t s0, size_t b) { return s0 == 0 ? (size_t)-1 : (size_t)s0 * b - 1; }

// Where the groups' head rows lie in the compact buffers.  base[gi] = heads before group gi, base[n_groups] = all heads.
enum { REPROVE_MAX_GROUPS = 16 };
struct ReproveLayout {
    size_t U[REPROVE_MAX_GROUPS];                // head rows of each group (0: the group launches nothing)
    size_t party_off[REPROVE_MAX_GROUPS];        // its parties in the compact [U][m] arrays
    size_t word_off[REPROVE_MAX_GROUPS];         // its proofs in the compact proof buffer (32-bit words)
    size_t parties, words, heads;                // totals
};
static void reprove_layout(uint32_t n_groups, const uint32_t* base, const uint32_t* m, const uint32_t* pieces, ReproveLayout& L) {
    L = ReproveLayout{};
    for (uint32_t gi = 0; gi < n_groups; gi++) {
        L.U[gi] = (size_t)base[gi + 1] - (size_t)base[gi];
        L.party_off[gi] = L.parties; L.word_off[gi] = L.words;
        L.parties += L.U[gi] * (size_t)m[gi]; L.words += L.U[gi] * (size_t)pieces[gi] * 4;
    }
    L.heads = base[n_groups];
}
