// Dapol::remove_ids (include/dapol.hpp) against libdapol_hip.so: after the removal a removed id has no proof, a kept one has, and the
// root equals dapol_tree_build over the kept (index, value, blinding) triples with the same seed.  The triples come from
// dapol_build_leaf_nodes over the same liabilities -- not from Dapol::create over the kept ones, whose collision resolution depends
// on the input order and could move an entity.  Without a GPU it prints NO_DEVICE and exits 0.
#include <cstdio>
#include <set>
#include <string>
#include "dapol.hpp"

int main() {
    using namespace dapol;
    std::shared_ptr<Context> ctx;
    try {
        ctx = std::make_shared<Context>(0, 16);
    } catch (const DapolError& e) {
        if (e.code == DAPOL_ERR_NO_DEVICE) { std::printf("NO_DEVICE %s\n", e.what()); return 0; }
        std::printf("FAIL ctx %d\n", e.code);
        return 1;
    }
    const int height = 16, n = 40;
    std::vector<Liability> liab;
    for (int i = 0; i < n; i++)
        liab.push_back({liability_id_from_str("user-" + std::to_string(i)), liability_id_from_str("ext-" + std::to_string(i)), (uint64_t)(3 * i + 1)});
    DapolOptions opt;
    opt.audit_seed = {'r', 'e', 'm', 'o', 'v', 'e'};
    opt.tree_height = height;
    opt.aggregation_factor = height;
    for (int i = 0; i < 32; i++) opt.secret[i] = (uint8_t)(7 * i + 1);
    Dapol d = Dapol::create(ctx, DAPOL_DIGEST_BLAKE3, liab, opt);

    // the leaves Dapol::create built: the same derivation, called directly
    std::vector<uint8_t> iid, eid;
    std::vector<uint32_t> ioff(n + 1, 0), eoff(n + 1, 0), order(n);
    std::vector<uint64_t> vals(n), idx(n), v(n), by_entity(n);
    std::vector<Bytes32> r(n);
    for (int i = 0; i < n; i++) {
        iid.insert(iid.end(), liab[i].internal_id.begin(), liab[i].internal_id.end());
        eid.insert(eid.end(), liab[i].external_id.begin(), liab[i].external_id.end());
        ioff[i + 1] = (uint32_t)iid.size();
        eoff[i + 1] = (uint32_t)eid.size();
        vals[i] = liab[i].value;
    }
    check(dapol_build_leaf_nodes(ctx->get(), DAPOL_DIGEST_BLAKE3, opt.audit_seed.data(), opt.audit_seed.size(), height, n, iid.data(), ioff.data(),
                                 eid.data(), eoff.data(), vals.data(), idx.data(), v.data(), r[0].data(), order.data(), by_entity.data()));

    const std::vector<int> gone_ent = {0, 1, 7, 8, 9, 23, 39};
    std::vector<LiabilityId> gone;
    std::set<uint64_t> gone_idx;
    for (int e : gone_ent) { gone.push_back(liab[e].internal_id); gone_idx.insert(by_entity[e]); }
    const DapolNode before = d.root_raw();
    try {                                                          // an unknown id: nothing is removed
        std::vector<LiabilityId> bad = gone;
        bad.push_back(liability_id_from_str("nobody"));
        d.remove_ids(bad);
        std::printf("FAIL unknown id accepted\n");
        return 1;
    } catch (const DapolError& e) {
        if (e.code != DAPOL_ERR_UNKNOWN_LEAF) { std::printf("FAIL unknown id code %d\n", e.code); return 1; }
    }
    const DapolNode same = d.root_raw();
    if (same.com != before.com || same.hash != before.hash || d.id_to_idx_map().size() != (size_t)n) { std::printf("FAIL unknown id changed the tree\n"); return 1; }

    d.remove_ids(gone);
    if (d.id_to_idx_map().size() != (size_t)(n - gone.size())) { std::printf("FAIL id map\n"); return 1; }
    Bytes32 nonce;
    for (int i = 0; i < 32; i++) nonce[i] = (uint8_t)i;
    for (auto& id : gone)
        if (d.generate_proof_for_id(id, nonce, 8)) { std::printf("FAIL proof for a removed id\n"); return 1; }
    auto kept = d.generate_proof_for_id(liab[2].internal_id, nonce, 8);
    if (!kept || kept->leaf_index != by_entity[2] || kept->merkle_siblings.size() != (size_t)height) { std::printf("FAIL proof for a kept id\n"); return 1; }

    std::vector<uint64_t> ki, kv;
    std::vector<Bytes32> kr;
    uint64_t sum = 0;
    for (int p = 0; p < n; p++)
        if (!gone_idx.count(idx[p])) { ki.push_back(idx[p]); kv.push_back(v[p]); kr.push_back(r[p]); sum += v[p]; }
    dapol_tree* t = nullptr;
    check(dapol_tree_build(ctx->get(), height, ki.size(), ki.data(), kv.data(), kr[0].data(), opt.secret.data(), 0, &t));
    DapolNode want;
    check(dapol_tree_root(t, want.com.data(), want.hash.data(), &want.v, want.v_blinding.data()));
    dapol_tree_destroy(t);
    const DapolNode got = d.root_raw();
    if (got.com != want.com || got.hash != want.hash || got.v != want.v || got.v_blinding != want.v_blinding || got.v != sum) {
        std::printf("FAIL root differs from the build over the kept leaves\n");
        return 1;
    }
    std::printf("OK remove kept=%zu root_value=%llu\n", ki.size(), (unsigned long long)got.v);
    return 0;
}
