// Dapol::generate_proofs_compact / verify_proofs_compact / CompactProofs::expand (include/dapol.hpp) against libdapol_hip.so: the
// expansion equals generate_proofs_shared's proofs byte for byte, the compact form is shorter than the blobs, it verifies with as many
// range proofs checked as the plan has distinct statements, and one flipped byte of a shared sub-proof fails exactly the proofs that
// use it.  Without a GPU it prints NO_DEVICE and exits 0.
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

    auto shared = d.generate_proofs_shared(idx, seed, n_bits);
    auto compact = d.generate_proofs_compact(idx, seed, n_bits);
    if (!shared || !compact) { std::printf("FAIL generate\n"); return 1; }
    uint64_t planned = 0;
    check(dapol_shared_plan(height, n, idx.data(), (int)Policy::Padding, (int)agg, nullptr, &planned, nullptr));
    const size_t es = dapol_entity_proof_size(height, (int)Policy::Padding, (int)agg, n_bits);
    if (compact->unique != planned || compact->compact.size() >= (size_t)n * es) { std::printf("FAIL compact size\n"); return 1; }
    auto all = compact->expand();
    for (int i = 0; i < n; i++) {
        if (all[i].range_proofs != (*shared)[i].range_proofs || all[i].leaf_index != idx[i]) { std::printf("FAIL expansion of %d\n", i); return 1; }
        for (int s = 0; s < height; s++)
            if (all[i].merkle_siblings[s].com != (*shared)[i].merkle_siblings[s].com || all[i].merkle_siblings[s].hash != (*shared)[i].merkle_siblings[s].hash) {
                std::printf("FAIL path of %d\n", i);
                return 1;
            }
    }
    auto one = compact->expand(17, 1);                              // one user's proof, verified on its own
    if (one.size() != 1 || one[0].range_proofs != (*shared)[17].range_proofs || !one[0].verify(*ctx, d.root(), leaves[17])) { std::printf("FAIL expand(17, 1)\n"); return 1; }

    auto res = Dapol::verify_proofs_compact(*ctx, d.root(), leaves, *compact, seed.data());
    for (int i = 0; i < n; i++)
        if (!res.first[i]) { std::printf("FAIL proof %d does not verify\n", i); return 1; }
    if (res.second != planned || res.second >= (uint64_t)n * 7) { std::printf("FAIL unique %llu planned %llu\n", (unsigned long long)res.second, (unsigned long long)planned); return 1; }

    // leaves 0 .. 63 of this height-8 tree lie under one depth-2 node: compact proof 0 is the aggregated proof of entities 0 .. 23
    Dapol::CompactProofs bad = *compact;
    bad.compact[40] ^= 0x01;
    auto res2 = Dapol::verify_proofs_compact(*ctx, d.root(), leaves, bad);               // (a seed from the OS)
    auto bad_all = bad.expand();
    for (int i = 0; i < n; i++) {
        const bool same = bad_all[i].range_proofs == (*shared)[i].range_proofs;
        if (res2.first[i] != same) { std::printf("FAIL tampered: verdict of %d is %d\n", i, (int)res2.first[i]); return 1; }
        if (same != (i >= 24)) { std::printf("FAIL tampered: proof 0 is used by other rows than expected (%d)\n", i); return 1; }
    }
    bad.compact.pop_back();                                         // a buffer of the wrong length: all invalid, no over-read
    auto res3 = Dapol::verify_proofs_compact(*ctx, d.root(), leaves, bad);
    for (int i = 0; i < n; i++)
        if (res3.first[i]) { std::printf("FAIL wrong length accepted\n"); return 1; }
    std::printf("OK compact n=%d unique=%llu of %d bytes=%zu of %zu\n", n, (unsigned long long)res.second, n * 7, compact->compact.size(), (size_t)n * es);
    return 0;
}
