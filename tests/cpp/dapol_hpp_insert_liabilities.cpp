// Dapol::insert_liabilities (include/dapol.hpp) against libdapol_hip.so: create over 100 liabilities, then 10 more join by id.  At
// height 8 (110 leaves in 256 slots) many of the new ids meet an old leaf on their walk, so the equality that is checked -- the root
// and the id map are those of create over all 110 -- holds only if the tree's leaves count as taken.  An id that is in the map already
// throws DuplicatedInternalId with map and root unchanged; the proof of a new id verifies.  Without a GPU it prints NO_DEVICE and
// exits 0.
#include <cstdio>
#include <string>
#include "dapol.hpp"

using namespace dapol;

static bool same(const DapolNode& a, const DapolNode& b) { return a.com == b.com && a.hash == b.hash && a.v == b.v && a.v_blinding == b.v_blinding; }

int main() {
    std::shared_ptr<Context> ctx;
    try {
        ctx = std::make_shared<Context>(0, 16);
    } catch (const DapolError& e) {
        if (e.code == DAPOL_ERR_NO_DEVICE) { std::printf("NO_DEVICE %s\n", e.what()); return 0; }
        std::printf("FAIL ctx %d\n", e.code);
        return 1;
    }
    const int height = 8, n0 = 100, k = 10, n = n0 + k;
    std::vector<Liability> all;
    for (int i = 0; i < n; i++)
        all.push_back({liability_id_from_str("user-" + std::to_string(i)), liability_id_from_str("ext-" + std::to_string(i)), (uint64_t)(i % 7 + 1)});
    const std::vector<Liability> old(all.begin(), all.begin() + n0), fresh(all.begin() + n0, all.end());
    DapolOptions opt;
    opt.audit_seed = {'j', 'o', 'i', 'n'};
    opt.tree_height = height;
    opt.aggregation_factor = height;
    for (int i = 0; i < 32; i++) opt.secret[i] = (uint8_t)(5 * i + 3);
    const Dapol want = Dapol::create(ctx, DAPOL_DIGEST_BLAKE3, all, opt);
    Dapol d = Dapol::create(ctx, DAPOL_DIGEST_BLAKE3, old, opt);

    const DapolNode before = d.root_raw();
    for (int twice = 0; twice < 2; twice++) {                       // an id the map holds already / an id given twice: nothing happens
        std::vector<Liability> bad = fresh;
        bad.push_back(twice ? fresh[3] : old[17]);
        try {
            d.insert_liabilities(bad);
            std::printf("FAIL duplicated id accepted (%d)\n", twice);
            return 1;
        } catch (const DapolError& e) {
            if (e.code != DAPOL_ERR_DUPLICATED_INTERNAL_ID) { std::printf("FAIL duplicated id code %d\n", e.code); return 1; }
        }
        if (!same(d.root_raw(), before) || d.id_to_idx_map().size() != (size_t)n0) { std::printf("FAIL a refused insert changed the Dapol\n"); return 1; }
    }
    try {                                                           // no audit seed to derive with
        Dapol blank = Dapol::new_blank(ctx, height, height);
        blank.insert_liabilities(fresh);
        std::printf("FAIL a blank Dapol accepted ids\n");
        return 1;
    } catch (const DapolError& e) {
        if (e.code != DAPOL_ERR_INVALID_ARGUMENT) { std::printf("FAIL blank code %d\n", e.code); return 1; }
    }

    d.insert_liabilities(fresh);
    if (d.id_to_idx_map().size() != (size_t)n || d.id_to_idx_map() != want.id_to_idx_map()) { std::printf("FAIL id map\n"); return 1; }
    const DapolNode got = d.root_raw();
    if (!same(got, want.root_raw())) { std::printf("FAIL root differs from create over all liabilities\n"); return 1; }

    // the proof of a new id verifies against its leaf node (blinding: the same derivation, called directly)
    std::vector<uint8_t> iid, eid;
    std::vector<uint32_t> ioff(n + 1, 0), eoff(n + 1, 0), order(n);
    std::vector<uint64_t> vals(n), idx(n), v(n), by_entity(n);
    std::vector<Bytes32> r(n);
    for (int i = 0; i < n; i++) {
        iid.insert(iid.end(), all[i].internal_id.begin(), all[i].internal_id.end());
        eid.insert(eid.end(), all[i].external_id.begin(), all[i].external_id.end());
        ioff[i + 1] = (uint32_t)iid.size();
        eoff[i + 1] = (uint32_t)eid.size();
        vals[i] = all[i].value;
    }
    check(dapol_build_leaf_nodes(ctx->get(), DAPOL_DIGEST_BLAKE3, opt.audit_seed.data(), opt.audit_seed.size(), height, n, iid.data(), ioff.data(),
                                 eid.data(), eoff.data(), vals.data(), idx.data(), v.data(), r[0].data(), order.data(), by_entity.data()));
    Bytes32 nonce;
    for (int i = 0; i < 32; i++) nonce[i] = (uint8_t)(i + 9);
    const int e = n0 + 4;
    auto proof = d.generate_proof_for_id(all[e].internal_id, nonce, 16);
    size_t p = 0;
    while (p < (size_t)n && order[p] != (uint32_t)e) p++;
    if (!proof || p == (size_t)n || proof->leaf_index != by_entity[e] || idx[p] != by_entity[e]) { std::printf("FAIL proof for a new id\n"); return 1; }
    if (!proof->verify(*ctx, d.root(), ctx->node_new(all[e].value, r[p]).get_proof_node())) { std::printf("FAIL the proof of a new id does not verify\n"); return 1; }
    std::printf("OK insert_liabilities leaves=%zu root_value=%llu\n", d.id_to_idx_map().size(), (unsigned long long)got.v);
    return 0;
}
