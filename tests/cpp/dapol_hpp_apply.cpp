// Dapol::apply and Dapol::apply_liabilities (include/dapol.hpp) against libdapol_hip.so.  By index: a mixed change set -- leaves removed,
// a sibling pair and scattered leaves added, liabilities replaced -- gives the root of dapol_tree_build over the resulting (index, value,
// blinding) triples with the same seed, and says which puts were new; a change set with one bad part (a removal that is no leaf, an
// index both removed and put) throws with NOTHING applied.  By id: ids leave and join in one edit, the id map follows only when the
// library call succeeds, and the root is that of the three separate calls.  Without a GPU it prints NO_DEVICE and exits 0.
#include <cstdio>
#include <map>
#include <string>
#include "dapol.hpp"

using namespace dapol;

static Bytes32 blinding(uint64_t x) {
    Bytes32 r{};
    for (int i = 0; i < 31; i++) r[i] = (uint8_t)(x * 37 + i * 11 + 5);
    return r;
}
static DapolNode built(const std::shared_ptr<Context>& ctx, int height, const std::map<uint64_t, uint64_t>& leaves, const Bytes32& seed) {
    std::vector<uint64_t> idx, v;
    std::vector<Bytes32> r;
    for (auto& kv : leaves) { idx.push_back(kv.first); v.push_back(kv.second); r.push_back(blinding(kv.first + kv.second)); }
    dapol_tree* t = nullptr;
    check(dapol_tree_build(ctx->get(), height, idx.size(), idx.data(), v.data(), r[0].data(), seed.data(), 0, &t));
    DapolNode n;
    check(dapol_tree_root(t, n.com.data(), n.hash.data(), &n.v, n.v_blinding.data()));
    dapol_tree_destroy(t);
    return n;
}
static bool same(const DapolNode& a, const DapolNode& b) { return a.com == b.com && a.hash == b.hash && a.v == b.v && a.v_blinding == b.v_blinding; }
template <typename F>
static int thrown(F&& f) {
    try { f(); } catch (const DapolError& e) { return e.code; }
    return 0;
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
    // ---- by index
    const int height = 16;
    Bytes32 seed;
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(7 * i + 1);
    std::map<uint64_t, uint64_t> leaves;                             // index -> value; the blinding is blinding(index + value)
    for (uint64_t i = 0; i < 100; i++) leaves[(i * 1597 + 13) % 65536 | 1024] = 3 * i + 1;      // (none in 512 .. 519 or at 40000 / 40001)
    std::vector<uint64_t> idx, v;
    std::vector<Bytes32> r;
    for (auto& kv : leaves) { idx.push_back(kv.first); v.push_back(kv.second); r.push_back(blinding(kv.first + kv.second)); }
    Dapol d = Dapol::new_blank(ctx, height, height);
    d.build(idx, v, r, seed);
    const DapolNode before = d.root_raw();

    const std::vector<uint64_t> gone = {idx[3], idx[50], idx[51], idx[3]};                       // (a duplicate removes its leaf once)
    std::vector<uint64_t> pi = {40001, idx[7], 512, 40000, idx[90], 517}, pv;
    std::vector<Bytes32> pr;
    for (uint64_t x : pi) { pv.push_back(x % 97 + 2); pr.push_back(blinding(x + pv.back())); }
    // one bad part refuses the whole change set
    std::vector<uint64_t> bad_gone = gone;
    bad_gone.push_back(600);                                         // not a leaf
    if (thrown([&] { d.apply(bad_gone, pi, pv, pr); }) != DAPOL_ERR_UNKNOWN_LEAF) { std::printf("FAIL unknown removal\n"); return 1; }
    if (thrown([&] { d.apply({idx[7]}, pi, pv, pr); }) != DAPOL_ERR_INVALID_ARGUMENT) { std::printf("FAIL removed and put\n"); return 1; }
    if (thrown([&] { d.apply(idx, {}, {}, {}); }) != DAPOL_ERR_INVALID_ARGUMENT) { std::printf("FAIL empty result\n"); return 1; }
    if (!same(d.root_raw(), before)) { std::printf("FAIL a refused apply changed the tree\n"); return 1; }
    if (!d.apply({}, {}, {}, {}).empty() || !same(d.root_raw(), before)) { std::printf("FAIL the empty apply\n"); return 1; }

    const std::vector<bool> was_new = d.apply(gone, pi, pv, pr);
    if (was_new != std::vector<bool>{true, false, true, true, false, true}) { std::printf("FAIL was_new\n"); return 1; }
    for (uint64_t x : gone) leaves.erase(x);
    for (size_t i = 0; i < pi.size(); i++) leaves[pi[i]] = pv[i];
    const DapolNode got = d.root_raw();
    if (!same(got, built(ctx, height, leaves, seed))) { std::printf("FAIL root differs from the build over the edited leaf set\n"); return 1; }
    // ---- by id
    const int h8 = 8, n0 = 60, k = 6, n = n0 + k;
    std::vector<Liability> all;
    for (int i = 0; i < n; i++)
        all.push_back({liability_id_from_str("user-" + std::to_string(i)), liability_id_from_str("ext-" + std::to_string(i)), (uint64_t)(i % 7 + 1)});
    const std::vector<Liability> old(all.begin(), all.begin() + n0), fresh(all.begin() + n0, all.end());
    DapolOptions opt;
    opt.audit_seed = {'m', 'i', 'x'};
    opt.tree_height = h8;
    opt.aggregation_factor = h8;
    for (int i = 0; i < 32; i++) opt.secret[i] = (uint8_t)(5 * i + 3);
    Dapol a = Dapol::create(ctx, DAPOL_DIGEST_BLAKE3, old, opt), b = Dapol::create(ctx, DAPOL_DIGEST_BLAKE3, old, opt);
    const std::vector<LiabilityId> leaving = {old[4].internal_id, old[5].internal_id, old[33].internal_id};
    const DapolNode a0 = a.root_raw();
    const auto map0 = a.id_to_idx_map();
    std::vector<LiabilityId> unknown = leaving;
    unknown.push_back(liability_id_from_str("nobody"));
    std::vector<Liability> dup = fresh;
    dup.push_back(old[17]);
    std::vector<Liability> back = fresh;
    back.push_back(old[4]);                                          // an id that leaves in this very call is still taken
    if (thrown([&] { a.apply_liabilities(unknown, fresh); }) != DAPOL_ERR_UNKNOWN_LEAF || thrown([&] { a.apply_liabilities(leaving, dup); }) != DAPOL_ERR_DUPLICATED_INTERNAL_ID ||
        thrown([&] { a.apply_liabilities(leaving, back); }) != DAPOL_ERR_DUPLICATED_INTERNAL_ID) { std::printf("FAIL id refusals\n"); return 1; }
    if (!same(a.root_raw(), a0) || a.id_to_idx_map() != map0) { std::printf("FAIL a refused apply_liabilities changed the Dapol\n"); return 1; }
    a.apply_liabilities(leaving, fresh);
    b.insert_liabilities(fresh);                                     // the same indexes: both derive against the old leaves
    b.remove_ids(leaving);
    if (a.id_to_idx_map() != b.id_to_idx_map() || a.id_to_idx_map().size() != (size_t)(n - 3)) { std::printf("FAIL id map\n"); return 1; }
    if (!same(a.root_raw(), b.root_raw())) { std::printf("FAIL apply_liabilities differs from insert_liabilities + remove_ids\n"); return 1; }
    std::printf("OK apply leaves=%zu root_value=%llu ids=%zu\n", leaves.size(), (unsigned long long)got.v, a.id_to_idx_map().size());
    return 0;
}
