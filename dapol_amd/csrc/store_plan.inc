// dapol_proof_store as index arithmetic: the lower bound the store's kernels search their sorted leaf indexes with, the alignment of a
// new leaf set against the rows the store holds (which old row a new row continues, if any) and the byte sizes of a store's buffers.
// Pure functions, no HIP call and no context: the kernels (kernels_store.h) and the host side (host_store.inc) call them, and
// tests/cpp/store_plan_asan.cpp replays them on the CPU under ASan + UBSan (tests/test_store_plan_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define STP_HD __host__ __device__ __forceinline__
#else
#define STP_HD inline
#endif

enum : uint32_t { STORE_NONE = 0xffffffffu };      // "no row": a store holds fewer than 2^32 rows (entities x plan size stays below 2^32)

// The first position of the strictly increasing idx[0 .. n) whose value is not below x (n: none is).
STP_HD size_t store_lower_bound(const uint64_t* idx, size_t n, uint64_t x) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (idx[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The row that holds leaf x, or STORE_NONE.
STP_HD uint32_t store_row_of(const uint64_t* idx, size_t n, uint64_t x) {
    const size_t at = store_lower_bound(idx, n, x);
    return at < n && idx[at] == x ? (uint32_t)at : (uint32_t)STORE_NONE;
}

// The alignment k_store_align computes, restated for the host: src[e] = the old row of new leaf e (STORE_NONE: it has none),
// has_old[e] = 1 where it has one.  Returns the rows with old data -- what a refresh reports as moved_rows when rows move, and what
// decides between its two paths: the leaf set is unchanged exactly when n_old == b == the return value (both arrays ascend strictly).
static inline size_t store_align_host(size_t n_old, const uint64_t* old_idx, size_t b, const uint64_t* new_idx, uint32_t* src, uint8_t* has_old) {
    size_t with_old = 0;
    for (size_t e = 0; e < b; e++) {
        const uint32_t row = store_row_of(old_idx, n_old, new_idx[e]);
        if (src) src[e] = row;
        if (has_old) has_old[e] = row != STORE_NONE ? 1 : 0;
        with_old += row != STORE_NONE ? 1 : 0;
    }
    return with_old;
}
static inline bool store_same_leaf_set(size_t n_old, size_t b, size_t with_old) { return n_old == b && with_old == b; }

// Bytes of a store's buffers for `rows` rows of H siblings: the leaf indexes, ONE set of sibling commitments and hashes (the store
// keeps two: a refresh gathers the new paths into the spare set and compares them with the other), the blobs.
struct StoreBytes {
    size_t idx = 0, path_C = 0, path_H = 0, range = 0;
    size_t resident() const { return idx + 2 * (path_C + path_H) + range; }           // between calls, both sibling sets allocated
    size_t move_transient() const { return range + path_C; }                          // a row-moving refresh: the second blob buffer and the compare buffer
};
static inline StoreBytes store_bytes(size_t rows, int H, size_t hash_bytes, size_t entity_bytes) {
    StoreBytes B;
    B.idx = rows * 8;
    B.path_C = rows * (size_t)H * 32;
    B.path_H = rows * (size_t)H * hash_bytes;
    B.range = rows * entity_bytes;
    return B;
}
// 16-byte pieces of one row: its blob, its commitments, its hashes (what k_store_fetch strides over).
STP_HD size_t store_row_pieces(size_t entity_pieces, int H, int hash_words) { return entity_pieces + 2 * (size_t)H + (size_t)H * (size_t)hash_words / 4; }
