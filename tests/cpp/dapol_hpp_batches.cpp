// Dapol::generate_proof_batches / DapolBatchProof::verify_many (include/dapol.hpp) against libdapol_hip.so: the proofs of one call
// equal generate_proof_batch's one by one, all verify in one call, a tampered one fails alone, an unknown leaf gives nullopt.  Without
// a GPU it prints NO_DEVICE and exits 0.
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
    const size_t agg = 2;
    std::vector<uint64_t> idx(n), v(n);
    std::vector<Bytes32> r(n);
    for (int i = 0; i < n; i++) {
        idx[i] = (uint64_t)(i < 24 ? i : 100 + 3 * i);             // a dense corner (pairs and whole subtrees) and scattered leaves
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
    auto leaf_of = [&](uint64_t x) {
        DapolProofNode l;
        for (int i = 0; i < n; i++)
            if (idx[i] == x) { std::memcpy(l.com.data(), &lC[i * 32], 32); std::memcpy(l.hash.data(), &lH[i * 32], 32); }
        return l;
    };

    // one leaf, a sibling pair, a whole subtree, scattered leaves, an overlap and a repeat
    const std::vector<std::vector<uint64_t>> batches = {{5}, {4, 5}, {8, 9, 10, 11}, {3, 172, 190}, {5, 9, 175}, {4, 5}, {217}, {0, 1, 2, 3, 4, 5, 6, 7}};
    auto proofs = d.generate_proof_batches(batches, seed, n_bits);
    if (!proofs || proofs->size() != batches.size()) { std::printf("FAIL generate_proof_batches: %s\n", dapol_last_error()); return 1; }
    std::vector<std::vector<DapolProofNode>> leaves(batches.size());
    for (size_t j = 0; j < batches.size(); j++) {
        for (uint64_t x : batches[j]) leaves[j].push_back(leaf_of(x));
        auto one = d.generate_proof_batch(batches[j], seed, n_bits);
        const DapolBatchProof& p = (*proofs)[j];
        if (!one || one->range_proofs != p.range_proofs || one->merkle_siblings.size() != p.merkle_siblings.size() || one->leaf_indexes != p.leaf_indexes) {
            std::printf("FAIL batch %zu differs from generate_proof_batch\n", j);
            return 1;
        }
        for (size_t s = 0; s < p.merkle_siblings.size(); s++)
            if (one->merkle_siblings[s].com != p.merkle_siblings[s].com || one->merkle_siblings[s].hash != p.merkle_siblings[s].hash) {
                std::printf("FAIL batch %zu sibling %zu\n", j, s);
                return 1;
            }
    }
    auto ok = DapolBatchProof::verify_many(*ctx, d.root(), *proofs, leaves, seed);
    for (size_t j = 0; j < ok.size(); j++)
        if (!ok[j] || !(*proofs)[j].verify_batch(*ctx, d.root(), leaves[j], seed)) { std::printf("FAIL batch %zu does not verify\n", j); return 1; }

    std::vector<DapolBatchProof> bad = *proofs;
    bad[3].range_proofs[40] ^= 0x01;                               // a flipped byte
    bad[1].merkle_siblings.pop_back();                             // a proof of the wrong shape
    bad[6].n_bits = 16;                                            // a proof of another call's shape
    auto ok2 = DapolBatchProof::verify_many(*ctx, d.root(), bad, leaves);      // (a seed from the OS)
    for (size_t j = 0; j < ok2.size(); j++)
        if (ok2[j] != (j != 3 && j != 1 && j != 6)) { std::printf("FAIL tampered: verdict of %zu is %d\n", j, (int)ok2[j]); return 1; }

    if (d.generate_proof_batches({{5}, {4, 5, 99}}, seed, n_bits)) { std::printf("FAIL unknown leaf\n"); return 1; }
    if (!d.generate_proof_batches({}, seed, n_bits)->empty() || !DapolBatchProof::verify_many(*ctx, d.root(), {}, {}).empty()) { std::printf("FAIL empty call\n"); return 1; }
    std::printf("OK batches n=%zu\n", batches.size());
    return 0;
}
