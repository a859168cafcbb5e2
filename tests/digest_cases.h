// The SHA-256 / SHA3-256 cases of tests/digest_host_shim.cpp (host, loaded by the tests), tests/cpp/digest_asan.cpp (host, under the
// sanitizers) and tests/digest_dev_shim.hip (gfx950), written once: dapol_amd/csrc/hash.h as the library compiles it.
// kind = 4 (DG_SHA256) or 5 (DG_SHA3_256), the DAPOL_DIGEST_* ids.
#pragma once
#include <stddef.h>
#include "../dapol_amd/csrc/hash.h"

namespace dapol_test {
using namespace dapol;

// The streaming digest of msg[0 .. n), fed in pieces of `piece` bytes (0: one call of dg_update); msg == nullptr: the counter pattern
// msg[i] = (uint8_t)i, fed byte by byte.
template <class D>
DAPOL_HD void digest_stream_as(int kind, const uint8_t* msg, size_t n, size_t piece, uint32_t* out8) {
    D d;
    dg_init(d, kind);
    if (!msg) {
        for (size_t i = 0; i < n; i++) dg_update_byte(d, (uint8_t)i);
    } else if (piece == 0) {
        dg_update(d, msg, (uint32_t)n);
    } else {
        for (size_t o = 0; o < n; o += piece) dg_update(d, msg + o, (uint32_t)(n - o < piece ? n - o : piece));
    }
    dg_final(d, out8);
}
DAPOL_HD void digest_stream(int kind, const uint8_t* msg, size_t n, size_t piece, uint32_t* out8) {
    if (kind == DG_SHA256) digest_stream_as<Sha256Stream>(kind, msg, n, piece, out8);
    else digest_stream_as<Sha3Stream>(kind, msg, n, piece, out8);
}
// Both node hashes of one input of 32 words: out32 = D(in[0 .. 8)), out128 = D(in[0 .. 32)) as C_L, C_R, H_L, H_R.
DAPOL_HD void digest_nodes(int kind, const uint32_t* in32, uint32_t* out32, uint32_t* out128) {
    if (kind == DG_SHA256) {
        node_hash_leaf_w<8, DG_SHA256>(kind, out32, in32);
        node_hash_parent_w<8, DG_SHA256>(kind, out128, in32, in32 + 8, in32 + 16, in32 + 24);
    } else {
        node_hash_leaf_w<8, DG_SHA3_256>(kind, out32, in32);
        node_hash_parent_w<8, DG_SHA3_256>(kind, out128, in32, in32 + 8, in32 + 16, in32 + 24);
    }
}

}  // namespace dapol_test
