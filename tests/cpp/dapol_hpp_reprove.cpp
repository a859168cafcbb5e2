// Dapol::regenerate_proofs_shared (include/dapol.hpp) against libdapol_hip.so: with the proofs of generate_proofs_shared as old proofs and
// nothing edited it proves nothing and returns them; after an update, an insert of two leaves and a removal it returns exactly what
// generate_proofs_shared gives on the edited tree while proving fewer range proofs, and every proof verifies; without old proofs it is
// the shared call; a leaf that is not there gives nullopt.  Without a GPU it prints NO_DEVICE and exits 0.
#include <cstdio>
#include <map>
#include "dapol.hpp"

using namespace dapol;

static Bytes32 blinding(uint64_t x) {
    Bytes32 r{};
    for (int i = 0; i < 31; i++) r[i] = (uint8_t)(x * 37 + i * 11 + 5);
    return r;
}
static bool same(const std::vector<DapolProof>& a, const std::vector<DapolProof>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].leaf_index != b[i].leaf_index || !(a[i].merkle_siblings == b[i].merkle_siblings) || a[i].range_proofs != b[i].range_proofs) return false;
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
    Dapol d = Dapol::new_blank(ctx, height, 4, Policy::Padding);               // a 4-party proof + 12 individual ones per entity
    d.build(idx, v, r, seed);
    const auto old = d.generate_proofs_shared(idx, nonce);
    if (!old) { std::printf("FAIL the shared call found no leaf\n"); return 1; }

    auto none = d.regenerate_proofs_shared(idx, *old, nonce);                   // nothing edited: nothing proved, the old proofs come back
    if (!none || none->second != 0 || !same(none->first, *old)) { std::printf("FAIL an unedited tree proved something\n"); return 1; }

    const uint64_t upd = idx[40], gone = idx[7], new_a = idx[40] ^ 1, new_b = 5;       // (indexes are all >= 1024 and odd multiples apart: both are free)
    if (leaves.count(new_a) || leaves.count(new_b)) { std::printf("FAIL the test's new leaves exist already\n"); return 1; }
    leaves[upd] = {777, blinding(upd + 1)};
    d.update(upd, leaves[upd].first, leaves[upd].second);
    leaves[new_a] = {11, blinding(new_a)}; leaves[new_b] = {12, blinding(new_b)};
    d.insert({new_a, new_b}, {11, 12}, {blinding(new_a), blinding(new_b)});
    leaves.erase(gone);
    d.remove({gone});
    arrays(idx, v, r);

    const auto fresh = d.generate_proofs_shared(idx, nonce);
    const auto again = d.regenerate_proofs_shared(idx, *old, nonce);
    const auto scratch = d.regenerate_proofs_shared(idx, {}, nonce);
    if (!fresh || !again || !scratch) { std::printf("FAIL a leaf of the edited tree was not found\n"); return 1; }
    if (!same(again->first, *fresh)) { std::printf("FAIL re-proved proofs differ from the shared call on the edited tree\n"); return 1; }
    if (!same(scratch->first, *fresh)) { std::printf("FAIL re-proving without old proofs differs from the shared call\n"); return 1; }
    if (again->second == 0 || again->second >= scratch->second) {
        std::printf("FAIL proved %llu, from scratch %llu\n", (unsigned long long)again->second, (unsigned long long)scratch->second);
        return 1;
    }
    const DapolProofNode root = d.root();
    for (size_t e = 0; e < idx.size(); e++)
        if (!again->first[e].verify(*ctx, root, ctx->node_new(v[e], r[e]).get_proof_node())) { std::printf("FAIL proof %zu does not verify\n", e); return 1; }
    std::vector<uint64_t> with_hole = {idx[0], idx[0] + 2};
    if (leaves.count(idx[0] + 2) || d.regenerate_proofs_shared(with_hole, *old, nonce)) { std::printf("FAIL an unknown leaf was proved\n"); return 1; }
    std::printf("OK reprove leaves=%zu proved=%llu of %llu\n", idx.size(), (unsigned long long)again->second, (unsigned long long)scratch->second);
    return 0;
}
