// dapol_batch_store as index arithmetic: which old row a batch of a new list CONTINUES (the lowest old row whose leaf list equals the
// new batch's in length and in every index), whether a new list is the stored one row for row, the staging offsets of a fetch, and
// where a 16-byte piece of a moved or fetched row comes from.  Pure functions, no HIP call and no context: the kernels
// (kernels_batch_store.h) and the host side (host_batch_store.inc) call them, and tests/cpp/batch_store_plan_asan.cpp replays them on
// the CPU under ASan + UBSan (tests/test_batch_store_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define BSP_HD __host__ __device__ __forceinline__
#else
#define BSP_HD inline
#endif

enum : uint32_t { BATCH_STORE_NONE = 0xffffffffu };      // "no old row": a store holds fewer than 2^32 batches

// Leaf lists in lexicographic order, a proper prefix before the longer list: < 0, 0, > 0.
static inline int batch_store_compare(const uint64_t* a, size_t na, const uint64_t* b, size_t nb) {
    const size_t n = na < nb ? na : nb;
    for (size_t i = 0; i < n; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na == nb ? 0 : (na < nb ? -1 : 1);
}

// src[j] = the LOWEST old row whose leaf list equals new batch j's, or BATCH_STORE_NONE; has_old[j] = 1 where there is one (either
// output may be null).  Returns the batches that continue an old row: what a moving refresh reports as moved_rows.  The old rows are
// sorted once by (list, row); every new batch is one binary search.  Offsets are dapol_prove_batches' (off[0] = 0, non-decreasing).
static inline size_t batch_store_match(size_t n_old, const uint64_t* old_off, const uint64_t* old_leaf, size_t nb, const uint64_t* new_off,
                                       const uint64_t* new_leaf, uint32_t* src, uint8_t* has_old) {
    std::vector<uint32_t> order(n_old);
    for (size_t r = 0; r < n_old; r++) order[r] = (uint32_t)r;
    auto list = [&](const uint64_t* off, const uint64_t* leaf, size_t r, size_t& n) {
        n = (size_t)(off[r + 1] - off[r]);
        return n ? leaf + off[r] : nullptr;
    };
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        size_t nx, ny;
        const uint64_t *a = list(old_off, old_leaf, x, nx), *b = list(old_off, old_leaf, y, ny);
        const int c = batch_store_compare(a, nx, b, ny);
        return c ? c < 0 : x < y;
    });
    size_t with_old = 0;
    for (size_t j = 0; j < nb; j++) {
        size_t nj;
        const uint64_t* want = list(new_off, new_leaf, j, nj);
        size_t lo = 0, hi = n_old;                              // the first sorted old row whose list is not below batch j's
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            size_t nm;
            const uint64_t* have = list(old_off, old_leaf, order[mid], nm);
            if (batch_store_compare(have, nm, want, nj) < 0) lo = mid + 1; else hi = mid;
        }
        uint32_t row = BATCH_STORE_NONE;
        if (lo < n_old) {
            size_t nm;
            const uint64_t* have = list(old_off, old_leaf, order[lo], nm);
            if (batch_store_compare(have, nm, want, nj) == 0) row = order[lo];
        }
        if (src) src[j] = row;
        if (has_old) has_old[j] = row != BATCH_STORE_NONE ? 1 : 0;
        with_old += row != BATCH_STORE_NONE ? 1 : 0;
    }
    return with_old;
}

// Is the new list the stored one, row for row?  (Then a refresh works in place; a permutation of the same batches does not.)
static inline bool batch_store_same_list(size_t n_old, const uint64_t* old_off, const uint64_t* old_leaf, size_t nb, const uint64_t* new_off,
                                         const uint64_t* new_leaf) {
    if (n_old != nb) return false;
    for (size_t j = 0; j <= nb; j++)
        if (old_off[j] != new_off[j]) return false;
    for (size_t i = 0, K = nb ? (size_t)new_off[nb] : 0; i < K; i++)
        if (old_leaf[i] != new_leaf[i]) return false;
    return true;
}

// The staging layout of a fetch: query i = row[i] of a store whose rows lie at sib_off / range_off (dapol_batches_plan's, [rows + 1],
// sibling records and bytes).  q_sib_off / q_piece_off [k + 1] = where query i's sibling records and 16-byte blob pieces start in the
// staging arrays -- dapol_batches_plan's offsets of those batches in query order (range bytes / 16).  false: a row number >= rows
// (nothing written beyond what came before it).
static inline bool batch_store_fetch_offsets(size_t k, const uint64_t* row, size_t rows, const uint64_t* sib_off, const uint64_t* range_off, uint64_t* q_sib_off,
                                             uint64_t* q_piece_off) {
    for (size_t i = 0; i < k; i++)
        if (row[i] >= rows) return false;
    q_sib_off[0] = 0; q_piece_off[0] = 0;
    for (size_t i = 0; i < k; i++) {
        const size_t r = (size_t)row[i];
        q_sib_off[i + 1] = q_sib_off[i] + (sib_off[r + 1] - sib_off[r]);
        q_piece_off[i + 1] = q_piece_off[i] + (range_off[r + 1] - range_off[r]) / 16;
    }
    return true;
}

// The last row with off[row] <= x (rows that own nothing before it are skipped); off [rows + 1], off[0] = 0 <= x < off[rows].
BSP_HD size_t batch_store_row(const uint64_t* off, size_t rows, uint64_t x) {
    size_t lo = 0, hi = rows;
    while (hi - lo > 1) {
        const size_t mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Piece t of a destination array whose row d owns [dst_off[d], dst_off[d + 1]) x unit pieces and is a copy of source row from[d]
// (BATCH_STORE_NONE: of none), which starts at src_off[from[d]] x unit: the source piece, or SIZE_MAX where the row has no source.
// The move reads from = the continuation table and dst_off / src_off = the new / old offsets; the fetch from = the queried rows and
// dst_off / src_off = the staging / the store's offsets.  unit = 1 for blob pieces, 2 for 32-byte records.
BSP_HD size_t batch_store_piece_src(size_t t, uint32_t unit, size_t rows, const uint64_t* dst_off, const uint32_t* from, const uint64_t* src_off) {
    const size_t d = batch_store_row(dst_off, rows, (uint64_t)(t / unit));
    const uint32_t r = from[d];
    if (r == BATCH_STORE_NONE) return (size_t)-1;
    return (size_t)src_off[r] * unit + (t - (size_t)dst_off[d] * unit);
}
