// Dapol::proof_store (include/dapol.hpp) against libdapol_hip.so: a store filled by refresh() serves the proofs of generate_proofs_shared;
// after an update a refresh proves fewer range proofs than the fill, moves no row, and proof(leaf) equals regenerate_proofs_shared's
// proof of that leaf; after an insert and a removal the rows move and the proofs are again the shared call's; verify() holds after
// every refresh and fails before it; a leaf the store does not hold gives nullopt; the store outlives the Dapol it came from.
// Without a GPU it prints NO_DEVICE and exits 0.
#include <cstdio>
#include <map>
#include "dapol.hpp"

using namespace dapol;

static Bytes32 blinding(uint64_t x) {
    Bytes32 r{};
    for (int i = 0; i < 31; i++) r[i] = (uint8_t)(x * 37 + i * 11 + 5);
    return r;
}
static bool same(const DapolProof& a, const DapolProof& b) {
    return a.leaf_index == b.leaf_index && a.merkle_siblings == b.merkle_siblings && a.range_proofs == b.range_proofs && a.policy == b.policy &&
           a.aggregation_factor == b.aggregation_factor && a.n_bits == b.n_bits && a.height == b.height;
}
static bool serves(const ProofStore& st, const std::vector<uint64_t>& idx, const std::vector<DapolProof>& want) {
    const auto got = st.proofs(idx);
    if (got.size() != want.size()) return false;
    for (size_t e = 0; e < want.size(); e++)
        if (!got[e] || !same(*got[e], want[e])) return false;
    return true;
}

int main() {
    std::shared_ptr<Context> ctx;
    try {
        ctx = std::make_shared<Context>(0, 16);
    } catch (const DapolError& e) {
        if (e.code == DAPOL_ERR_NO_DEVICE) { std::printf("NO_DEVICE %s\n", e.what()); return 0; }
        std::printf("FAIL ctx %d\n", e.code);
        return 1;
    }
    const int height = 16;
    Bytes32 seed, nonce;
    for (int i = 0; i < 32; i++) { seed[i] = (uint8_t)(7 * i + 1); nonce[i] = (uint8_t)(5 * i + 3); }
    std::map<uint64_t, std::pair<uint64_t, Bytes32>> leaves;                    // index -> (value, blinding)
    for (uint64_t i = 0; i < 100; i++) { const uint64_t x = (i * 1597 + 13) % 65536 | 1024; leaves[x] = {3 * i + 1, blinding(x)}; }
    auto arrays = [&](std::vector<uint64_t>& idx, std::vector<uint64_t>& v, std::vector<Bytes32>& r) {
        idx.clear(); v.clear(); r.clear();
        for (auto& kv : leaves) { idx.push_back(kv.first); v.push_back(kv.second.first); r.push_back(kv.second.second); }
    };
    std::vector<uint64_t> idx, v;
    std::vector<Bytes32> r;
    arrays(idx, v, r);
    std::unique_ptr<Dapol> d(new Dapol(Dapol::new_blank(ctx, height, 4, Policy::Padding)));       // a 4-party proof + 12 individual ones per entity
    d->build(idx, v, r, seed);
    const auto old = d->generate_proofs_shared(idx, nonce);
    if (!old) { std::printf("FAIL the shared call found no leaf\n"); return 1; }

    ProofStore made = d->proof_store(nonce);
    if (made.rows() != 0 || made.verify()) { std::printf("FAIL a new store is not empty\n"); return 1; }
    ProofStore st = std::move(made);                                             // move-only: the handle travels
    const auto fill = st.refresh();
    if (st.rows() != idx.size() || fill.kept != 0 || fill.moved_rows != 0 || fill.proved == 0) { std::printf("FAIL the fill\n"); return 1; }
    if (!serves(st, idx, *old) || !st.verify()) { std::printf("FAIL the filled store differs from the shared call\n"); return 1; }
    const auto idle = st.refresh();
    if (idle.proved != 0 || idle.moved_rows != 0) { std::printf("FAIL an unedited tree proved something\n"); return 1; }

    const uint64_t upd = idx[40];
    leaves[upd] = {777, blinding(upd + 1)};
    d->update(upd, leaves[upd].first, leaves[upd].second);
    if (st.verify()) { std::printf("FAIL a stale store verifies\n"); return 1; }
    const auto again = d->regenerate_proofs_shared(idx, *old, nonce);
    const auto up = st.refresh();
    if (!again || up.proved != again->second || up.proved == 0 || up.proved >= fill.proved || up.moved_rows != 0) {
        std::printf("FAIL the refresh after an update proved %llu\n", (unsigned long long)up.proved);
        return 1;
    }
    for (size_t e : {(size_t)0, (size_t)40, idx.size() - 1}) {
        const auto p = st.proof(idx[e]);
        if (!p || !same(*p, again->first[e])) { std::printf("FAIL proof(%zu) differs from regenerate_proofs_shared's\n", e); return 1; }
    }
    if (!serves(st, idx, again->first) || !st.verify()) { std::printf("FAIL the refreshed store\n"); return 1; }

    const uint64_t gone = idx[7], new_a = idx[40] ^ 1, new_b = 5;
    if (leaves.count(new_a) || leaves.count(new_b)) { std::printf("FAIL the test's new leaves exist already\n"); return 1; }
    leaves[new_a] = {11, blinding(new_a)}; leaves[new_b] = {12, blinding(new_b)};
    d->insert({new_a, new_b}, {11, 12}, {blinding(new_a), blinding(new_b)});
    leaves.erase(gone);
    d->remove({gone});
    arrays(idx, v, r);
    const auto fresh = d->generate_proofs_shared(idx, nonce);
    const auto mv = st.refresh();
    if (!fresh || mv.moved_rows != idx.size() - 2 || st.rows() != idx.size() || !serves(st, idx, *fresh) || !st.verify()) {
        std::printf("FAIL the refresh after insert + remove\n");
        return 1;
    }
    if (st.proof(gone) || st.proof(7)) { std::printf("FAIL a leaf that is not held was served\n"); return 1; }
    const DapolProofNode root = d->root();
    const auto mine = st.proof(new_b);
    if (!mine || !mine->verify(*ctx, root, ctx->node_new(12, blinding(new_b)).get_proof_node())) { std::printf("FAIL the served proof does not verify\n"); return 1; }

    const auto sub = st.refresh({idx[1], idx[3]});
    if (st.rows() != 2 || sub.moved_rows != 2 || sub.proved != 0 || !st.verify()) { std::printf("FAIL a subset\n"); return 1; }
    d.reset();                                                                   // the store shares the tree: it stays usable
    if (!st.proof(idx[3]) || st.proof(idx[2]) || !st.verify()) { std::printf("FAIL the store after its Dapol went\n"); return 1; }
    if (st.refresh({}).moved_rows != 0 || st.rows() != 0) { std::printf("FAIL emptying\n"); return 1; }
    std::printf("OK store leaves=%zu fill=%llu update=%llu moved=%llu\n", idx.size(), (unsigned long long)fill.proved, (unsigned long long)up.proved,
                (unsigned long long)mv.moved_rows);
    return 0;
}
