// Dapol::batch_store (include/dapol.hpp) against libdapol_hip.so: a store filled by refresh(batches) serves the proofs of
// generate_proof_batches; after an update a refresh() proves what regenerate_proof_batches proves, moves no row, and the served proofs
// equal its proofs; after a removal a refresh() reports the lost leaf and leaves the store alone, and the list without the lost batch
// (and with a new one) moves the surviving rows; verify() holds after every refresh and fails before it; the store outlives the Dapol
// it came from.  Without a GPU it prints NO_DEVICE and exits 0.
#include <cstdio>
#include <map>
#include "dapol.hpp"

using namespace dapol;

static Bytes32 blinding(uint64_t x) {
    Bytes32 r{};
    for (int i = 0; i < 31; i++) r[i] = (uint8_t)(x * 37 + i * 11 + 5);
    return r;
}
static bool same(const DapolBatchProof& a, const DapolBatchProof& b) {
    return a.leaf_indexes == b.leaf_indexes && a.merkle_siblings == b.merkle_siblings && a.range_proofs == b.range_proofs && a.policy == b.policy &&
           a.aggregation_factor == b.aggregation_factor && a.n_bits == b.n_bits && a.height == b.height;
}
static bool serves(const BatchProofStore& st, const std::vector<DapolBatchProof>& want) {
    std::vector<uint64_t> rows;
    for (size_t j = want.size(); j-- > 0;) rows.push_back(j);                     // backwards, and the first row once more
    rows.push_back(0);
    const auto got = st.proofs(rows);
    if (st.rows() != want.size() || got.size() != rows.size()) return false;
    for (size_t i = 0; i < rows.size(); i++)
        if (!same(got[i], want[rows[i]])) return false;
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
    std::unique_ptr<Dapol> d(new Dapol(Dapol::new_blank(ctx, height, 4, Policy::Padding)));       // a 4-party proof + individual ones per batch
    d->build(idx, v, r, seed);
    std::vector<std::vector<uint64_t>> batches;                                  // customers with 1, 2, 3 accounts; one of them twice
    for (size_t i = 0; i + 3 <= 60; i += 3) batches.push_back(std::vector<uint64_t>(idx.begin() + i, idx.begin() + i + 1 + (i / 3) % 3));
    batches.push_back(batches[4]);
    const auto old = d->generate_proof_batches(batches, nonce);
    if (!old) { std::printf("FAIL generate_proof_batches found no leaf\n"); return 1; }

    BatchProofStore made = d->batch_store(nonce);
    if (made.rows() != 0 || made.verify()) { std::printf("FAIL a new store is not empty\n"); return 1; }
    BatchProofStore st = std::move(made);                                        // move-only: the handle travels
    const auto fill = st.refresh(batches);
    if (!fill || st.rows() != batches.size() || fill->kept != 0 || fill->moved_rows != 0 || fill->proved == 0 || st.batches() != batches) {
        std::printf("FAIL the fill\n");
        return 1;
    }
    if (!serves(st, *old) || !st.verify()) { std::printf("FAIL the filled store differs from generate_proof_batches\n"); return 1; }
    const auto idle = st.refresh();
    if (idle.proved != 0 || idle.n_calls != 0 || idle.moved_rows != 0) { std::printf("FAIL an unedited tree proved something\n"); return 1; }

    const uint64_t upd = idx[40];
    leaves[upd] = {777, blinding(upd + 1)};
    d->update(upd, leaves[upd].first, leaves[upd].second);
    if (st.verify()) { std::printf("FAIL a stale store verifies\n"); return 1; }
    const auto again = d->regenerate_proof_batches(*old, nonce);
    const auto up = st.refresh();
    if (!again || up.proved != again->second || up.proved == 0 || up.proved >= fill->proved || up.moved_rows != 0) {
        std::printf("FAIL the refresh after an update proved %llu\n", (unsigned long long)up.proved);
        return 1;
    }
    if (!serves(st, again->first) || !st.verify()) { std::printf("FAIL the refreshed store\n"); return 1; }

    const uint64_t gone = batches[2][0];
    leaves.erase(gone);
    d->remove({gone});
    try {
        st.refresh();
        std::printf("FAIL a refresh of a list that lost a leaf went through\n");
        return 1;
    } catch (const DapolError& e) {
        if (e.code != DAPOL_ERR_UNKNOWN_LEAF) { std::printf("FAIL a lost leaf gave code %d\n", e.code); return 1; }
    }
    if (st.refresh({batches[2]}) || st.rows() != batches.size() || !serves(st, again->first)) { std::printf("FAIL a lost leaf changed the store\n"); return 1; }
    std::vector<std::vector<uint64_t>> next;
    for (auto& b : batches)
        if (std::find(b.begin(), b.end(), gone) == b.end()) next.push_back(b);
    next.insert(next.begin() + 5, std::vector<uint64_t>{idx[70], idx[71]});
    const size_t lost = batches.size() + 1 - next.size();
    const auto fresh = d->generate_proof_batches(next, nonce);
    const auto mv = st.refresh(next);
    if (!fresh || !mv || lost == 0 || mv->moved_rows != next.size() - 1 || !serves(st, *fresh) || !st.verify()) {
        std::printf("FAIL the refresh after a removal\n");
        return 1;
    }
    const DapolProofNode root = d->root();
    const DapolBatchProof mine = st.proof(5);
    std::vector<DapolProofNode> mine_leaves;
    for (uint64_t x : mine.leaf_indexes) mine_leaves.push_back(ctx->node_new(leaves[x].first, leaves[x].second).get_proof_node());
    if (!mine.verify_batch(*ctx, root, mine_leaves)) { std::printf("FAIL the served proof does not verify\n"); return 1; }

    d.reset();                                                                   // the store shares the tree: it stays usable
    if (!same(st.proof(5), (*fresh)[5]) || !st.verify()) { std::printf("FAIL the store after its Dapol went\n"); return 1; }
    const auto none = st.refresh(std::vector<std::vector<uint64_t>>{});
    if (!none || none->moved_rows != 0 || st.rows() != 0) { std::printf("FAIL emptying\n"); return 1; }
    std::printf("OK batch_store batches=%zu fill=%llu update=%llu moved=%llu\n", batches.size(), (unsigned long long)fill->proved, (unsigned long long)up.proved,
                (unsigned long long)mv->moved_rows);
    return 0;
}
