// Dapol::verify_proofs_shared (include/dapol.hpp) against libdapol_hip.so: the proofs of generate_proofs_shared all verify with fewer
// range proofs checked than there are sub-proofs; one tampered copy of a shared sub-proof fails exactly its own entity.  Without a GPU
// it prints NO_DEVICE and exits 0.
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

    auto proofs = d.generate_proofs_shared(idx, seed, n_bits);
    if (!proofs || proofs->size() != (size_t)n) { std::printf("FAIL generate_proofs_shared\n"); return 1; }
    uint64_t planned = 0;
    check(dapol_shared_plan(height, n, idx.data(), (int)Policy::Padding, (int)agg, nullptr, &planned, nullptr));
    auto res = Dapol::verify_proofs_shared(*ctx, d.root(), leaves, *proofs, seed);
    for (int i = 0; i < n; i++)
        if (!res.first[i]) { std::printf("FAIL proof %d does not verify\n", i); return 1; }
    if (res.second != planned || res.second >= (uint64_t)n * 7) { std::printf("FAIL unique %llu planned %llu\n", (unsigned long long)res.second, (unsigned long long)planned); return 1; }
    for (int i = 0; i < n; i++)                                     // the same verdicts one by one
        if (!(*proofs)[i].verify(*ctx, d.root(), leaves[i])) { std::printf("FAIL DapolProof::verify %d\n", i); return 1; }

    // leaves 0 .. 3 share the aggregated proof (their two upper siblings are the same nodes): tamper entity 2's copy
    if ((*proofs)[1].range_proofs[40] != (*proofs)[2].range_proofs[40]) { std::printf("FAIL no shared bytes\n"); return 1; }
    std::vector<DapolProof> bad = *proofs;
    bad[2].range_proofs[40] ^= 0x01;
    auto res2 = Dapol::verify_proofs_shared(*ctx, d.root(), leaves, bad);            // (a seed from the OS)
    for (int i = 0; i < n; i++)
        if (res2.first[i] != (i != 2)) { std::printf("FAIL tampered: verdict of %d is %d\n", i, (int)res2.first[i]); return 1; }
    if (bad[2].verify(*ctx, d.root(), leaves[2])) { std::printf("FAIL tampered proof verifies alone\n"); return 1; }
    bad[5].merkle_siblings.pop_back();                             // a proof of the wrong shape: all invalid, no over-read
    auto res3 = Dapol::verify_proofs_shared(*ctx, d.root(), leaves, bad);
    for (int i = 0; i < n; i++)
        if (res3.first[i]) { std::printf("FAIL wrong shape accepted\n"); return 1; }
    std::printf("OK verify_shared n=%d unique=%llu of %d\n", n, (unsigned long long)res.second, n * 7);
    return 0;
}
