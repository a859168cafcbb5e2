// Dapol::generate_paths_compact / verify_proofs_compact_paths / CompactPaths::expand (include/dapol.hpp) against libdapol_hip.so: the
// expansion equals the Merkle siblings of generate_proofs_compact byte for byte, the compact paths hold fewer records than the
// per-entity ones, they verify with as many merges as records, and a non-canonical record fails exactly the proofs whose path holds it.
// Without a GPU it prints NO_DEVICE and exits 0.
#include <cstdio>
#include "dapol.hpp"

int main() {
    using namespace dapol;
    std::shared_ptr<Context> ctx;
    try {
        ctx = std::make_shared<Context>(0, 8);
    } catch (const DapolError& e) {
        if (e.code == DAPOL_ERR_NO_DEVICE) { std::printf("NO_DEVICE %s\n", e.what()); return 0; }
        std::printf("FAIL ctx %d\n", e.code);
        return 1;
    }
    const int height = 8, n = 40, n_bits = 8;
    const size_t agg = 2;                                          // padding: one 2-party proof + 6 individual ones per entity
    std::vector<uint64_t> idx(n), v(n);
    std::vector<Bytes32> r(n);
    for (int i = 0; i < n; i++) {
        idx[i] = (uint64_t)(i < 24 ? i : 100 + 3 * i);             // a dense corner (shared upper siblings) and scattered leaves
        v[i] = (uint64_t)(i % 5);
        for (int j = 0; j < 32; j++) r[i][j] = (uint8_t)(i * 31 + j * 7 + 1);
        r[i][31] &= 0x0F;
    }
    Bytes32 seed;
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 2);
    Dapol d = Dapol::new_blank(ctx, height, agg, Policy::Padding);
    d.build(idx, v, r, seed);
    std::vector<uint8_t> lC(n * 32), lH(n * 32);
    check(dapol_commit_hash_batch(ctx->get(), n, v.data(), r[0].data(), lC.data(), lH.data()));
    std::vector<DapolProofNode> leaves(n);
    for (int i = 0; i < n; i++) { std::memcpy(leaves[i].com.data(), &lC[i * 32], 32); std::memcpy(leaves[i].hash.data(), &lH[i * 32], 32); }

    auto compact = d.generate_proofs_compact(idx, seed, n_bits);
    auto paths = d.generate_paths_compact(idx);
    if (!compact || !paths) { std::printf("FAIL generate\n"); return 1; }
    uint64_t planned = 0;
    check(dapol_compact_paths_plan(height, n, idx.data(), nullptr, nullptr, &planned));
    if (paths->records() != planned || planned >= (uint64_t)n * height) { std::printf("FAIL record count\n"); return 1; }
    auto all = paths->expand();
    for (int i = 0; i < n; i++)
        for (int s = 0; s < height; s++)
            if (all[i][s].com != compact->merkle_siblings[i][s].com || all[i][s].hash != compact->merkle_siblings[i][s].hash) {
                std::printf("FAIL path of %d\n", i);
                return 1;
            }
    auto one = paths->expand(17, 1);                                // one user's path
    if (one.size() != 1 || one[0].size() != (size_t)height || one[0][3].com != compact->merkle_siblings[17][3].com) { std::printf("FAIL expand(17, 1)\n"); return 1; }
    std::vector<uint64_t> missing = {0, 1, 99};                    // no liability at leaf 99
    if (d.generate_paths_compact(missing)) { std::printf("FAIL unknown leaf accepted\n"); return 1; }

    auto res = Dapol::verify_proofs_compact_paths(*ctx, d.root(), leaves, *compact, *paths, seed.data());
    for (int i = 0; i < n; i++)
        if (!res.ok[i]) { std::printf("FAIL proof %d does not verify\n", i); return 1; }
    if (res.path_merges != planned || res.unique != compact->unique) {
        std::printf("FAIL merges %llu records %llu unique %llu\n", (unsigned long long)res.path_merges, (unsigned long long)planned, (unsigned long long)res.unique);
        return 1;
    }
    // the sibling of leaf 16 is the leaf of row 17, a record on row 16's path alone; row 17 joins row 16's chain one level up.  p itself
    // (s = 0 written non-canonically, RFC 9496) must fail row 16 and nothing else
    uint64_t depth_off[height + 2];
    std::vector<uint32_t> ref((size_t)height * n);
    check(dapol_compact_paths_plan(height, n, idx.data(), depth_off, ref.data(), nullptr));
    Dapol::CompactPaths bad = *paths;
    const size_t rec = (size_t)depth_off[height] + ref[(size_t)(height - 1) * n + 16];
    std::memset(&bad.com[rec * 32], 0xFF, 32);
    bad.com[rec * 32] = 0xED; bad.com[rec * 32 + 31] = 0x7F;
    auto res2 = Dapol::verify_proofs_compact_paths(*ctx, d.root(), leaves, *compact, bad);        // (a seed from the OS)
    for (int i = 0; i < n; i++)
        if (res2.ok[i] != (i != 16)) { std::printf("FAIL tampered: verdict of %d is %d\n", i, (int)res2.ok[i]); return 1; }
    if (res2.path_merges != planned + (uint64_t)n * height) { std::printf("FAIL tampered: merges %llu\n", (unsigned long long)res2.path_merges); return 1; }
    bad.com.resize(bad.com.size() - 32); bad.hash.resize(bad.hash.size() - 32);          // a buffer of the wrong length: all invalid, no over-read
    auto res3 = Dapol::verify_proofs_compact_paths(*ctx, d.root(), leaves, *compact, bad);
    for (int i = 0; i < n; i++)
        if (res3.ok[i]) { std::printf("FAIL wrong length accepted\n"); return 1; }
    std::printf("OK compact paths n=%d records=%llu of %d merges=%llu\n", n, (unsigned long long)planned, n * height, (unsigned long long)res.path_merges);
    return 0;
}
