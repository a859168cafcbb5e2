// include/dapol.hpp with the SHA-256 and SHA3-256 digests against libdapol_hip.so: Context refuses every id but 0, 1, 4 and 5 with
// DapolError(DAPOL_ERR_INVALID_DIGEST_SIZE) before the library is called (3 is reserved, 2 = Blake2b has 64-byte hashes), and
// Dapol::create under 4 and 5 maps the reference's KAT liabilities (ids a, b, c, d; external w, x, y, z; seed "test"; height 4) where
// the Python oracle with hashlib's digests does (tests/test_digests_cpu.py), with root value 26 and a proof for every id.
// Without a GPU it prints NO_DEVICE after the refusals and exits 0.
#include <cstdio>
#include <string>
#include "dapol.hpp"

int main() {
    using namespace dapol;
    for (int bad : {3, 6, -1, 2}) {
        try {
            Context c(0, 8, bad);
            std::printf("FAIL digest %d accepted\n", bad);
            return 1;
        } catch (const DapolError& e) {
            if (e.code != DAPOL_ERR_INVALID_DIGEST_SIZE) { std::printf("FAIL digest %d code %d\n", bad, e.code); return 1; }
        }
    }
    const struct { int digest; uint64_t index[4]; } want[2] = {{DAPOL_DIGEST_SHA256, {8, 15, 9, 2}}, {DAPOL_DIGEST_SHA3_256, {2, 15, 1, 4}}};
    const char* ids[4] = {"a", "b", "c", "d"};
    const char* ext[4] = {"w", "x", "y", "z"};
    const uint64_t values[4] = {3, 5, 7, 11};
    for (auto& w : want) {
        std::shared_ptr<Context> ctx;
        try {
            ctx = std::make_shared<Context>(0, 8, w.digest);
        } catch (const DapolError& e) {
            if (e.code == DAPOL_ERR_NO_DEVICE) { std::printf("NO_DEVICE %s\n", e.what()); return 0; }
            std::printf("FAIL ctx digest %d code %d\n", w.digest, e.code);
            return 1;
        }
        std::vector<Liability> liab;
        for (int i = 0; i < 4; i++) liab.push_back({liability_id_from_str(ids[i]), liability_id_from_str(ext[i]), values[i]});
        DapolOptions opt;
        opt.audit_seed = {'t', 'e', 's', 't'};
        opt.tree_height = 4;
        opt.aggregation_factor = 2;
        for (int i = 0; i < 32; i++) opt.secret[i] = (uint8_t)i;
        Dapol d = Dapol::create(ctx, w.digest, liab, opt);
        for (int i = 0; i < 4; i++) {
            auto it = d.id_to_idx_map().find(liab[i].internal_id);
            if (it == d.id_to_idx_map().end() || it->second != w.index[i]) { std::printf("FAIL digest %d id %s\n", w.digest, ids[i]); return 1; }
        }
        if (d.root_raw().v != 26) { std::printf("FAIL digest %d root value\n", w.digest); return 1; }
        Bytes32 nonce;
        for (int i = 0; i < 32; i++) nonce[i] = (uint8_t)i;
        for (int i = 0; i < 4; i++) {
            auto p = d.generate_proof_for_id(liab[i].internal_id, nonce, 8);
            if (!p || p->leaf_index != w.index[i] || p->merkle_siblings.size() != 4) { std::printf("FAIL digest %d proof %s\n", w.digest, ids[i]); return 1; }
        }
    }
    std::printf("OK digests 4 5\n");
    return 0;
}
