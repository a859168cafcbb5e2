// Dapol::regenerate_proof_batches (include/dapol.hpp) against libdapol_hip.so: with the proofs of generate_proof_batches as old proofs
// and nothing edited it proves nothing and returns them; after an update it returns exactly what generate_proof_batches gives on the
// edited tree while proving what regenerate_proof_batches_plan announces -- fewer range proofs than from scratch -- and every proof
// verifies; a batch without an old proof is proved whole; a leaf that is not there gives nullopt.  Without a GPU it prints NO_DEVICE
// and exits 0.
#include <cstdio>
#include <map>
#include "dapol.hpp"

using namespace dapol;

static Bytes32 blinding(uint64_t x) {
    Bytes32 r{};
    for (int i = 0; i < 31; i++) r[i] = (uint8_t)(x * 37 + i * 11 + 5);
    return r;
}
static bool same(const std::vector<DapolBatchProof>& a, const std::vector<DapolBatchProof>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].leaf_indexes != b[i].leaf_indexes || !(a[i].merkle_siblings == b[i].merkle_siblings) || a[i].range_proofs != b[i].range_proofs) return false;
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
    std::vector<uint64_t> idx, v;
    std::vector<Bytes32> r;
    for (auto& kv : leaves) { idx.push_back(kv.first); v.push_back(kv.second.first); r.push_back(kv.second.second); }
    Dapol d = Dapol::new_blank(ctx, height, 4, Policy::Padding);               // a 4-party proof + the individual ones per batch
    d.build(idx, v, r, seed);
    // batches of 1, 2 and 3 leaves, interleaved; the last two repeat and overlap
    std::vector<std::vector<uint64_t>> batches;
    for (size_t i = 0; i + 6 <= idx.size(); i += 6) {
        batches.push_back({idx[i]});
        batches.push_back({idx[i + 1], idx[i + 2]});
        batches.push_back({idx[i + 3], idx[i + 4], idx[i + 5]});
    }
    batches.push_back(batches[1]);
    batches.push_back({idx[1], idx[3], idx[40]});
    const auto old = d.generate_proof_batches(batches, nonce);
    if (!old) { std::printf("FAIL the batch call found no leaf\n"); return 1; }

    auto none = d.regenerate_proof_batches(*old, nonce);                        // nothing edited: nothing proved, the old proofs come back
    if (!none || none->second != 0 || !same(none->first, *old)) { std::printf("FAIL an unedited tree proved something\n"); return 1; }

    const uint64_t upd = idx[40];
    v[40] = 777; r[40] = blinding(upd + 1);
    d.update(upd, v[40], r[40]);
    const auto fresh = d.generate_proof_batches(batches, nonce);
    const auto again = d.regenerate_proof_batches(*old, nonce);
    std::vector<DapolBatchProof> bare(batches.size());                          // no old proofs: only the leaves
    for (size_t j = 0; j < batches.size(); j++) bare[j].leaf_indexes = batches[j];
    const auto scratch = d.regenerate_proof_batches(bare, nonce);
    std::vector<DapolBatchProof> mixed = *old;
    mixed[2] = bare[2];
    const auto part = d.regenerate_proof_batches(mixed, nonce);
    if (!fresh || !again || !scratch || !part) { std::printf("FAIL a leaf of the edited tree was not found\n"); return 1; }
    if (!same(again->first, *fresh)) { std::printf("FAIL re-proved batches differ from generate_proof_batches on the edited tree\n"); return 1; }
    if (!same(scratch->first, *fresh) || !same(part->first, *fresh)) { std::printf("FAIL re-proving without old proofs differs\n"); return 1; }
    const auto plan = d.regenerate_proof_batches_plan(batches, {upd});
    std::vector<uint8_t> flags(batches.size(), 1);
    flags[2] = 0;
    const auto plan_part = d.regenerate_proof_batches_plan(batches, {upd}, flags);
    if (again->second == 0 || again->second >= scratch->second || again->second != plan.proved || part->second != plan_part.proved ||
        plan.sum_m_proved >= plan.sum_m_all || plan.proved_per_batch.size() != batches.size()) {
        std::printf("FAIL proved %llu (plan %llu), from scratch %llu\n", (unsigned long long)again->second, (unsigned long long)plan.proved,
                    (unsigned long long)scratch->second);
        return 1;
    }
    const DapolProofNode root = d.root();
    std::map<uint64_t, size_t> at;
    for (size_t e = 0; e < idx.size(); e++) at[idx[e]] = e;
    for (size_t j = 0; j < batches.size(); j++) {
        std::vector<DapolProofNode> nodes;
        for (uint64_t x : batches[j]) nodes.push_back(ctx->node_new(v[at[x]], r[at[x]]).get_proof_node());
        if (!again->first[j].verify_batch(*ctx, root, nodes)) { std::printf("FAIL batch %zu does not verify\n", j); return 1; }
    }
    std::vector<DapolBatchProof> with_hole = {bare[0]};
    with_hole[0].leaf_indexes = {idx[0], idx[0] + 2};
    if (leaves.count(idx[0] + 2) || d.regenerate_proof_batches(with_hole, nonce)) { std::printf("FAIL an unknown leaf was proved\n"); return 1; }
    std::printf("OK reprove batches=%zu proved=%llu of %llu\n", batches.size(), (unsigned long long)again->second, (unsigned long long)scratch->second);
    return 0;
}
