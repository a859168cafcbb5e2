// SHA-256 / SHA3-256 of dapol_amd/csrc/hash.h (host build, tests/digest_cases.h) under AddressSanitizer + UBSan: the checks of
// tests/test_digests_cpu.py as a stand-alone program.  argv[1] = a file of expected answers that the test wrote with hashlib:
//   u32 n_len, n_len x u32 lengths, then per length the SHA-256 and the SHA3-256 (32 bytes each) of the counter pattern msg[i] = (u8)i;
//   u32 n_node, n_node x 128 input bytes, then per input SHA-256(in[..32]), SHA3-256(in[..32]), SHA-256(in), SHA3-256(in).
// Every message goes in one call and in pieces of 1, 7 and 64 bytes, from a heap buffer of exactly its length (a read past the end
// is the sanitizer's to find).  Prints "digest asan clean" and exits 0 when every digest matches.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../digest_cases.h"

static bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: digest_asan VECTORS\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    const int kinds[2] = {dapol::DG_SHA256, dapol::DG_SHA3_256};
    const size_t pieces[4] = {0, 1, 7, 64};
    uint32_t n_len = 0, n_node = 0;
    if (!read_exact(f, &n_len, 4) || n_len > 100000) { std::printf("bad vector file\n"); return 2; }
    std::vector<uint32_t> lens(n_len);
    std::vector<uint8_t> want((size_t)n_len * 64);
    if (!read_exact(f, lens.data(), 4 * (size_t)n_len) || !read_exact(f, want.data(), want.size())) { std::printf("bad vector file\n"); return 2; }
    size_t checked = 0;
    for (uint32_t i = 0; i < n_len; i++) {
        std::vector<uint8_t> msg(lens[i]);                       // exactly the message: no slack behind it
        for (size_t k = 0; k < msg.size(); k++) msg[k] = (uint8_t)k;
        for (int d = 0; d < 2; d++)
            for (size_t piece : pieces) {
                uint32_t out[8];
                dapol_test::digest_stream(kinds[d], msg.data(), msg.size(), piece, out);
                if (std::memcmp(out, &want[(size_t)i * 64 + 32 * d], 32) != 0) {
                    std::printf("FAIL stream kind %d length %u piece %zu\n", kinds[d], lens[i], piece);
                    return 1;
                }
                checked++;
            }
    }
    if (!read_exact(f, &n_node, 4) || n_node > 100000) { std::printf("bad vector file\n"); return 2; }
    std::vector<uint8_t> in((size_t)n_node * 128), wantn((size_t)n_node * 128);
    if (!read_exact(f, in.data(), in.size()) || !read_exact(f, wantn.data(), wantn.size())) { std::printf("bad vector file\n"); return 2; }
    std::fclose(f);
    for (uint32_t i = 0; i < n_node; i++) {
        std::vector<uint32_t> w(32);
        std::memcpy(w.data(), &in[(size_t)i * 128], 128);
        for (int d = 0; d < 2; d++) {
            uint32_t a[8], b[8];
            dapol_test::digest_nodes(kinds[d], w.data(), a, b);
            if (std::memcmp(a, &wantn[(size_t)i * 128 + 32 * d], 32) != 0 || std::memcmp(b, &wantn[(size_t)i * 128 + 64 + 32 * d], 32) != 0) {
                std::printf("FAIL node kind %d input %u\n", kinds[d], i);
                return 1;
            }
            checked += 2;
        }
    }
    std::printf("digest asan clean: %zu digests\n", checked);
    return 0;
}
