// The streaming SHA-256 / SHA3-256 digests and both node hashes of dapol_amd/csrc/hash.h compiled for the host (tests/digest_cases.h),
// for tests/test_digests_cpu.py to hold against hashlib and for tests/test_digests_gpu.py to hold the device's words against.
#include <stdint.h>
#include "digest_cases.h"

extern "C" {
// msg[0 .. n) in pieces of `piece` bytes (0: one call) -> 8 little-endian words = the digest's 32 bytes
void t_digest_stream(int kind, const uint8_t* msg, size_t n, size_t piece, uint32_t* out8) { dapol_test::digest_stream(kind, msg, n, piece, out8); }
// lane L of the device program: the L-byte counter pattern, byte by byte, L = 0 .. n - 1
void t_digest_stream_cases(int kind, int n, uint32_t* out /*[n][8]*/) {
    for (int l = 0; l < n; l++) dapol_test::digest_stream(kind, nullptr, (size_t)l, 0, out + 8 * l);
}
void t_digest_node_cases(int kind, int n, const uint32_t* in /*[n][32]*/, uint32_t* out32 /*[n][8]*/, uint32_t* out128 /*[n][8]*/) {
    for (int i = 0; i < n; i++) dapol_test::digest_nodes(kind, in + 32 * i, out32 + 8 * i, out128 + 8 * i);
}
}
