// Dapol::insert (include/dapol.hpp) against libdapol_hip.so: after a sibling pair and an aligned block of 8 have been inserted -- chains
// that share nodes -- the root equals dapol_tree_build over the old and the new (index, value, blinding) triples with the same seed; an
// index that is a leaf already throws DAPOL_ERR_INVALID_ARGUMENT with nothing inserted; a blank Dapol builds.  Without a GPU it prints
// NO_DEVICE and exits 0.
#include <cstdio>
#include <map>
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
    for (auto& kv : leaves) { idx.push_back(kv.first); v.push_back(kv.second); r.push_back(blinding(kv.first)); }
    dapol_tree* t = nullptr;
    check(dapol_tree_build(ctx->get(), height, idx.size(), idx.data(), v.data(), r[0].data(), seed.data(), 0, &t));
    DapolNode n;
    check(dapol_tree_root(t, n.com.data(), n.hash.data(), &n.v, n.v_blinding.data()));
    dapol_tree_destroy(t);
    return n;
}
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
    const int height = 16;
    Bytes32 seed;
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(7 * i + 1);
    std::map<uint64_t, uint64_t> leaves;
    for (uint64_t i = 0; i < 100; i++) leaves[(i * 1597 + 13) % 65536 | 1024] = 3 * i + 1;      // (none in 512 .. 519 or at 40000 / 40001)
    std::vector<uint64_t> idx, v;
    std::vector<Bytes32> r;
    for (auto& kv : leaves) { idx.push_back(kv.first); v.push_back(kv.second); r.push_back(blinding(kv.first)); }
    Dapol d = Dapol::new_blank(ctx, height, height);
    try {                                                            // a blank Dapol is all or nothing too: a duplicate builds nothing
        std::vector<uint64_t> bi = idx, bv = v;
        std::vector<Bytes32> br = r;
        bi.push_back(idx[5]); bv.push_back(1); br.push_back(blinding(1));
        d.insert(bi, bv, br, seed);
        std::printf("FAIL duplicate accepted by a blank Dapol\n");
        return 1;
    } catch (const DapolError& e) {
        if (e.code != DAPOL_ERR_INVALID_ARGUMENT) { std::printf("FAIL blank duplicate code %d\n", e.code); return 1; }
    }
    std::vector<uint64_t> ri(idx.rbegin(), idx.rend()), rv(v.rbegin(), v.rend());
    std::vector<Bytes32> rr(r.rbegin(), r.rend());
    d.insert(ri, rv, rr, seed);                                      // a blank Dapol builds, from any order
    if (!same(d.root_raw(), built(ctx, height, leaves, seed))) { std::printf("FAIL blank insert differs from the build\n"); return 1; }

    std::vector<uint64_t> ni = {40001, 519, 512, 40000, 517, 513, 516, 514, 518, 515}, nv;
    std::vector<Bytes32> nr;
    for (uint64_t x : ni) { nv.push_back(x % 97); nr.push_back(blinding(x)); }
    const DapolNode before = d.root_raw();
    try {                                                            // an index that is a leaf already: nothing is inserted
        std::vector<uint64_t> bi = ni;
        bi.push_back(idx[3]);
        std::vector<uint64_t> bv = nv;
        bv.push_back(1);
        std::vector<Bytes32> br = nr;
        br.push_back(blinding(1));
        d.insert(bi, bv, br);
        std::printf("FAIL existing index accepted\n");
        return 1;
    } catch (const DapolError& e) {
        if (e.code != DAPOL_ERR_INVALID_ARGUMENT) { std::printf("FAIL existing index code %d\n", e.code); return 1; }
    }
    if (!same(d.root_raw(), before)) { std::printf("FAIL a refused insert changed the tree\n"); return 1; }
    d.insert(ni, nv, nr);
    for (size_t i = 0; i < ni.size(); i++) leaves[ni[i]] = nv[i];
    const DapolNode got = d.root_raw();
    if (!same(got, built(ctx, height, leaves, seed))) { std::printf("FAIL root differs from the build over the union\n"); return 1; }
    std::printf("OK insert leaves=%zu root_value=%llu\n", leaves.size(), (unsigned long long)got.v);
    return 0;
}
