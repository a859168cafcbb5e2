// dapol.hpp -- C++ host-side mirror of the reference crate's public surface for the GPU proving path
// (src/lib.rs:1-11), over the C ABI of dapol_hip.h.  Same names, argument meaning and error behaviour:
//   Result<_, DapolError>  -> throws dapol::DapolError          (src/errors.rs:6-17)
//   Option<_>              -> std::optional                      (src/dapol/mod.rs:148-190)
//   panics                 -> throws dapol::DapolError{code 8}   (src/range/padding.rs:95-98, smtree build)
// Header-only; link with -ldapol_hip.  No computation happens here.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "dapol_hip.h"

namespace dapol {

using Bytes32 = std::array<uint8_t, 32>;

// utils::get_secret (src/utils.rs:19-26): 32 bytes from the OS CSPRNG.  Every seed of this API that hides something
// (padding blindings, prover nonces, verifier weights) is either passed explicitly or drawn here -- never a zero default.
inline Bytes32 get_secret() {
    Bytes32 s{};
    size_t got = 0;
    if (FILE* f = std::fopen("/dev/urandom", "rb")) {
        got = std::fread(s.data(), 1, s.size(), f);
        std::fclose(f);
    }
    if (got != s.size()) throw std::runtime_error("dapol: no OS randomness (/dev/urandom)");
    return s;
}

struct DapolError : std::runtime_error {      // src/errors.rs:6-17 (+ the ABI's extra codes)
    int32_t code;
    DapolError(int32_t c) : std::runtime_error(std::string(dapol_strerror(c)) + " [" + dapol_last_error() + "]"), code(c) {}
};
inline void check(int32_t rc) { if (rc != DAPOL_OK) throw DapolError(rc); }

// DapolProofNode<D> (src/proof/node.rs:17-22): commitment + hash, both 32 bytes (D = blake3::Hasher).
struct DapolProofNode {
    Bytes32 com{}, hash{};
    bool operator==(const DapolProofNode& o) const { return com == o.com && hash == o.hash; }   // src/proof/node.rs:24-29
};
// DapolNode<D> (src/dapol/node.rs:19-25) as it crosses the boundary: value, blinding, commitment, hash.
struct DapolNode {
    uint64_t v = 0;
    Bytes32 v_blinding{}, com{}, hash{};
    uint64_t get_value() const { return v; }
    const Bytes32& get_blinding() const { return v_blinding; }
    DapolProofNode get_proof_node() const { return {com, hash}; }      // ProofExtractable (node.rs:91-96)
    bool operator==(const DapolNode& o) const { return v == o.v; }     // node.rs:115-120: equal iff values are equal
};

class Context {                                // PedersenGens::default() + BulletproofGens::new(64, m), once
  public:
    // digest = the node hash D of Dapol<D, R>: DAPOL_DIGEST_BLAKE3, DAPOL_DIGEST_BLAKE2S, DAPOL_DIGEST_SHA256 or DAPOL_DIGEST_SHA3_256.  This mirror's node types carry 32-byte
    // hashes (Bytes32), like Dapol::new's DIGEST_SIZE check (src/dapol/mod.rs:101-103): the 64-byte DAPOL_DIGEST_BLAKE2B of the
    // new_blank + build path is served by the C ABI itself (include/dapol_hip.h), and is refused HERE before any buffer could be too small.
    // max_parties = the largest aggregation a proof may need, rounded up to a power of two: 32 serves trees up to height 32
    // (aggregation_factor <= tree_height), 64 the reference's whole range (MAX_TREE_HEIGHT = 64, src/dapol/mod.rs:26)
    explicit Context(int device = 0, int max_parties = 32, int digest = DAPOL_DIGEST_BLAKE3) { digest32(digest); check(dapol_ctx_create(device, max_parties, digest, &h_)); }
    // ... with settings (dapol_options: zeros = the library's own choices; options.struct_size is filled in here)
    Context(int device, int max_parties, int digest, dapol_options options) {
        digest32(digest);
        options.struct_size = (int32_t)sizeof(dapol_options);
        check(dapol_ctx_create_opts(device, max_parties, digest, &options, &h_));
    }
    dapol_options options() const { dapol_options o{}; check(dapol_ctx_get_options(h_, &o)); return o; }
    void set_options(dapol_options o) { o.struct_size = (int32_t)sizeof(dapol_options); check(dapol_ctx_set_options(h_, &o)); }
    ~Context() { dapol_ctx_destroy(h_); }
    static void digest32(int digest) {
        if (digest != DAPOL_DIGEST_BLAKE3 && digest != DAPOL_DIGEST_BLAKE2S && digest != DAPOL_DIGEST_SHA256 && digest != DAPOL_DIGEST_SHA3_256)
            throw DapolError(DAPOL_ERR_INVALID_DIGEST_SIZE);
    }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    dapol_ctx* get() const { return h_; }
    // DapolNode::new (src/dapol/node.rs:29-45)
    DapolNode node_new(uint64_t value, const Bytes32& blinding) const {
        DapolNode n;
        n.v = value;
        n.v_blinding = blinding;
        check(dapol_commit_hash_batch(h_, 1, &value, blinding.data(), n.com.data(), n.hash.data()));
        return n;
    }
    // Mergeable::merge (src/dapol/node.rs:64-80)
    DapolNode merge(const DapolNode& l, const DapolNode& r) const {
        DapolNode p;
        check(dapol_merge_batch(h_, 1, l.com.data(), l.hash.data(), &l.v, l.v_blinding.data(), r.com.data(), r.hash.data(), &r.v,
                                r.v_blinding.data(), p.com.data(), p.hash.data(), &p.v, p.v_blinding.data()));
        return p;
    }
  private:
    dapol_ctx* h_ = nullptr;
};

enum class Policy { Padding = DAPOL_POLICY_PADDING, Splitting = DAPOL_POLICY_SPLITTING };

// RangeProofPadding / RangeProofSplitting (src/range/padding.rs:20-23, splitting.rs:22-25): aggregated + individual proofs.
struct RangeProofs {
    Policy policy = Policy::Padding;
    std::vector<std::vector<uint8_t>> aggregated, individual;
};

// RangeProvable::generate_proof (src/range/mod.rs:29) for one sibling list, through the batched prover.
inline RangeProofs generate_proof(const Context& ctx, Policy policy, const std::vector<uint64_t>& secrets, const std::vector<Bytes32>& blindings,
                                  size_t aggregation_factor, const Bytes32& nonce_seed, uint64_t stream_id, int n_bits = 64) {
    if (aggregation_factor > secrets.size() || secrets.size() != blindings.size()) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
    RangeProofs out;
    out.policy = policy;
    uint64_t slot = 0;
    auto prove = [&](size_t start, size_t count, size_t m) {
        std::vector<uint64_t> v(m, 0);
        std::vector<uint8_t> r(m * 32, 0);
        for (size_t j = 0; j < m; j++) {
            if (j < count) { v[j] = secrets[start + j]; std::memcpy(&r[32 * j], blindings[start + j].data(), 32); }
            else r[32 * j] = 1;                                            // (0, Scalar::one())  padding.rs:100-103
        }
        std::vector<uint8_t> p(dapol_range_proof_size(n_bits, (int)m));
        check(dapol_range_prove_batch(ctx.get(), n_bits, (int)m, 1, v.data(), r.data(), nonce_seed.data(), &stream_id, slot, nullptr, p.data()));
        slot += m * (2 * (uint64_t)n_bits + 4);
        return p;
    };
    auto np2 = [](size_t x) { size_t p = 1; while (p < x) p <<= 1; return p; };
    if (policy == Policy::Padding) {
        out.aggregated.push_back(prove(0, aggregation_factor, np2(aggregation_factor)));
    } else {
        size_t base = np2(aggregation_factor), pos = 0;
        while (pos < aggregation_factor) {
            if (aggregation_factor & base) { out.aggregated.push_back(prove(pos, base, base)); pos += base; }
            base >>= 1;
        }
    }
    for (size_t i = aggregation_factor; i < secrets.size(); i++) out.individual.push_back(prove(i, 1, 1));
    return out;
}

// DapolProof::serialize / deserialize (src/proof/mod.rs:68-85): range_proof || merkle_path, shared by the two proof shapes
// below.  Deserialisation throws DapolError with DecodingError's codes (BytesNotEnough / ValueDecodingError); every sibling
// commitment is decompress-validated on the GPU (src/proof/node.rs:88-94).
inline std::vector<uint8_t> proof_serialize(int height, const std::vector<uint64_t>& leaves, const std::vector<DapolProofNode>& siblings, Policy policy,
                                            size_t aggregation_factor, int n_bits, const std::vector<uint8_t>& range_proofs) {
    size_t S = siblings.size(), n = dapol_proof_wire_size(height, leaves.size(), S, (int)policy, (int)aggregation_factor, n_bits);
    if (n == 0) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
    std::vector<uint8_t> C(S * 32 + 1), H(S * 32 + 1), wire(n);
    for (size_t i = 0; i < S; i++) { std::memcpy(&C[i * 32], siblings[i].com.data(), 32); std::memcpy(&H[i * 32], siblings[i].hash.data(), 32); }
    check(dapol_proof_serialize(height, leaves.size(), leaves.data(), S, C.data(), H.data(), (int)policy, (int)aggregation_factor, n_bits, range_proofs.data(),
                                wire.data()));
    return wire;
}
struct DecodedProof {
    int height = 0;
    size_t aggregation_factor = 0;
    std::vector<uint64_t> leaves;
    std::vector<DapolProofNode> siblings;
    std::vector<uint8_t> range_proofs;
};
inline DecodedProof proof_deserialize(const Context& ctx, Policy policy, int n_bits, const std::vector<uint8_t>& wire) {
    int32_t h = 0, agg = 0;
    size_t k = 0, S = 0, bl = 0;
    check(dapol_proof_deserialize(ctx.get(), (int)policy, n_bits, wire.data(), wire.size(), &h, &k, &S, &agg, &bl, nullptr, nullptr, nullptr, nullptr, nullptr));
    DecodedProof d;
    d.height = h; d.aggregation_factor = (size_t)agg;
    d.leaves.resize(k); d.siblings.resize(S); d.range_proofs.resize(bl);
    std::vector<uint8_t> C(S * 32 + 1), H(S * 32 + 1);
    std::vector<uint64_t> leaf(k + 1);
    std::vector<uint8_t> blob(bl + 1);
    check(dapol_proof_deserialize(ctx.get(), (int)policy, n_bits, wire.data(), wire.size(), &h, &k, &S, &agg, &bl, leaf.data(), C.data(), H.data(), blob.data(), nullptr));
    for (size_t i = 0; i < k; i++) d.leaves[i] = leaf[i];
    for (size_t i = 0; i < S; i++) { std::memcpy(d.siblings[i].com.data(), &C[i * 32], 32); std::memcpy(d.siblings[i].hash.data(), &H[i * 32], 32); }
    std::memcpy(d.range_proofs.data(), blob.data(), bl);
    return d;
}

// DapolProof<D, R> (src/proof/mod.rs:15-22) for single leaves: Merkle siblings (root side first) + range proofs.
struct DapolProof {
    uint64_t leaf_index = 0;
    std::vector<DapolProofNode> merkle_siblings;
    std::vector<uint8_t> range_proofs;           // aggregated proofs then individual proofs, concatenated
    Policy policy = Policy::Padding;
    size_t aggregation_factor = 0;
    int n_bits = 64, height = 0;
    std::vector<uint8_t> serialize() const { return proof_serialize(height, {leaf_index}, merkle_siblings, policy, aggregation_factor, n_bits, range_proofs); }
    static DapolProof deserialize(const Context& ctx, Policy policy, int n_bits, const std::vector<uint8_t>& wire) {
        DecodedProof d = proof_deserialize(ctx, policy, n_bits, wire);
        if (d.leaves.size() != 1) throw DapolError(DAPOL_ERR_VALUE_DECODING);
        DapolProof p;
        p.leaf_index = d.leaves[0]; p.merkle_siblings = std::move(d.siblings); p.range_proofs = std::move(d.range_proofs);
        p.policy = policy; p.aggregation_factor = d.aggregation_factor; p.n_bits = n_bits; p.height = d.height;
        return p;
    }
    // DapolProof::verify (src/proof/mod.rs:41-47)
    bool verify(const Context& ctx, const DapolProofNode& root, const DapolProofNode& leaf) const {
        size_t h = merkle_siblings.size();
        std::vector<uint8_t> C(h * 32 + 1), H(h * 32 + 1);
        for (size_t i = 0; i < h; i++) { std::memcpy(&C[i * 32], merkle_siblings[i].com.data(), 32); std::memcpy(&H[i * 32], merkle_siblings[i].hash.data(), 32); }
        uint8_t ok = 0;
        // the length-checked entry point: a proof whose sibling count or range-proof bytes do not fit (height, policy, aggregation
        // factor) -- e.g. one deserialised from hostile bytes -- is simply invalid
        check(dapol_verify_entities_checked(ctx.get(), height, 1, &leaf_index, leaf.com.data(), leaf.hash.data(), h, C.data(), H.data(), root.com.data(),
                                            root.hash.data(), (int)policy, (int)aggregation_factor, n_bits, range_proofs.data(), range_proofs.size(), nullptr, &ok));
        return ok != 0;
    }
};
// DapolProof<D, R> made by generate_proof_batch: MerkleProof::new_batch(leaf indexes) + the deduplicated siblings
// (level by level from the root side, left to right) + the range proofs over exactly those siblings.
struct DapolBatchProof {
    std::vector<uint64_t> leaf_indexes;
    std::vector<DapolProofNode> merkle_siblings;
    std::vector<uint8_t> range_proofs;
    Policy policy = Policy::Padding;
    size_t aggregation_factor = 0;
    int n_bits = 64, height = 0;
    std::vector<uint8_t> serialize() const { return proof_serialize(height, leaf_indexes, merkle_siblings, policy, aggregation_factor, n_bits, range_proofs); }
    static DapolBatchProof deserialize(const Context& ctx, Policy policy, int n_bits, const std::vector<uint8_t>& wire) {
        DecodedProof d = proof_deserialize(ctx, policy, n_bits, wire);
        DapolBatchProof p;
        p.leaf_indexes = std::move(d.leaves); p.merkle_siblings = std::move(d.siblings); p.range_proofs = std::move(d.range_proofs);
        p.policy = policy; p.aggregation_factor = d.aggregation_factor; p.n_bits = n_bits; p.height = d.height;
        return p;
    }
    // DapolProof::verify_batch (src/proof/mod.rs:49-54)
    // Without a seed the library draws the verifier's batching scalars' seed from the OS (the crate uses thread_rng).
    bool verify_batch(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves) const {
        return verify_batch_impl(ctx, root, leaves, nullptr);
    }
    bool verify_batch(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves, const Bytes32& verify_seed) const {
        return verify_batch_impl(ctx, root, leaves, verify_seed.data());
    }
    bool verify_batch_impl(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves, const uint8_t* verify_seed) const {
        if (leaves.size() != leaf_indexes.size()) return false;
        size_t k = leaves.size(), S = merkle_siblings.size();
        std::vector<uint8_t> lC(k * 32), lH(k * 32), sC(S * 32 + 1), sH(S * 32 + 1);
        for (size_t i = 0; i < k; i++) { std::memcpy(&lC[i * 32], leaves[i].com.data(), 32); std::memcpy(&lH[i * 32], leaves[i].hash.data(), 32); }
        for (size_t i = 0; i < S; i++) { std::memcpy(&sC[i * 32], merkle_siblings[i].com.data(), 32); std::memcpy(&sH[i * 32], merkle_siblings[i].hash.data(), 32); }
        uint8_t ok = 0;
        check(dapol_verify_batch_checked(ctx.get(), height, k, leaf_indexes.data(), lC.data(), lH.data(), S, sC.data(), sH.data(), root.com.data(),
                                         root.hash.data(), (int)policy, (int)aggregation_factor, n_bits, range_proofs.data(), range_proofs.size(), verify_seed, &ok));
        return ok != 0;
    }
    // verify_batch for MANY proofs in one call (dapol_verify_batches): out[j] is what proofs[j].verify_batch(ctx, root, leaves[j]) returns.
    // One call has one shape: a proof whose height, policy, aggregation factor or bit size differs from proofs[0]'s, or whose leaves do
    // not number its leaf indexes, is reported invalid and never changes another proof's verdict.  32-byte digests only.
    static std::vector<bool> verify_many(const Context& ctx, const DapolProofNode& root, const std::vector<DapolBatchProof>& proofs,
                                         const std::vector<std::vector<DapolProofNode>>& leaves, const uint8_t* verify_seed = nullptr) {
        if (leaves.size() != proofs.size()) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        std::vector<bool> out(proofs.size(), false);
        if (proofs.empty()) return out;
        const DapolBatchProof& f = proofs[0];
        std::vector<size_t> rows;
        std::vector<uint64_t> boff{0}, soff{0}, roff{0}, idx;
        std::vector<uint8_t> lC, lH, sC, sH, blob;
        auto put = [](std::vector<uint8_t>& to, const Bytes32& b) { to.insert(to.end(), b.begin(), b.end()); };
        for (size_t j = 0; j < proofs.size(); j++) {
            const DapolBatchProof& p = proofs[j];
            if (p.height != f.height || p.policy != f.policy || p.aggregation_factor != f.aggregation_factor || p.n_bits != f.n_bits ||
                leaves[j].size() != p.leaf_indexes.size())
                continue;
            rows.push_back(j);
            idx.insert(idx.end(), p.leaf_indexes.begin(), p.leaf_indexes.end());
            for (auto& l : leaves[j]) { put(lC, l.com); put(lH, l.hash); }
            for (auto& s : p.merkle_siblings) { put(sC, s.com); put(sH, s.hash); }
            blob.insert(blob.end(), p.range_proofs.begin(), p.range_proofs.end());
            boff.push_back(idx.size()); soff.push_back(sC.size() / 32); roff.push_back(blob.size());
        }
        std::vector<uint8_t> ok(rows.size() + 1, 0);
        lC.push_back(0); lH.push_back(0); sC.push_back(0); sH.push_back(0); blob.push_back(0); idx.push_back(0);      // (never NULL)
        check(dapol_verify_batches(ctx.get(), f.height, rows.size(), boff.data(), idx.data(), lC.data(), lH.data(), soff.data(), sC.data(), sH.data(),
                                   root.com.data(), root.hash.data(), (int)f.policy, (int)f.aggregation_factor, f.n_bits, roff.data(), blob.data(), verify_seed,
                                   ok.data()));
        for (size_t i = 0; i < rows.size(); i++) out[rows[i]] = ok[i] != 0;
        return out;
    }
    static std::vector<bool> verify_many(const Context& ctx, const DapolProofNode& root, const std::vector<DapolBatchProof>& proofs,
                                         const std::vector<std::vector<DapolProofNode>>& leaves, const Bytes32& verify_seed) {
        return verify_many(ctx, root, proofs, leaves, verify_seed.data());
    }
};

// LiabilityId / Liability / DapolOptions (src/dapol/mod.rs:36-56)
using LiabilityId = std::vector<uint8_t>;
inline LiabilityId liability_id_from_str(const std::string& s) { return LiabilityId(s.begin(), s.end()); }
struct Liability {
    LiabilityId internal_id, external_id;
    uint64_t value = 0;
};
struct DapolOptions {
    std::vector<uint8_t> audit_seed;
    int tree_height = 0;
    size_t aggregation_factor = 0;
    Bytes32 secret = get_secret();    // smtree Secret: here the seed of the positional padding draws.  Random unless the caller
                                      // sets it: a known seed makes every padding blinding publicly derivable (node.rs:86-88)
};

// dapol_proof_store: the proofs of Dapol::generate_proofs_shared kept on the GPU and re-proved in place after update / insert / remove
// (Dapol::proof_store makes one).  Move-only.  It shares ownership of the tree it was made on, and its destructor destroys the store
// before that share is dropped, so the tree outlives the store whatever becomes of the Dapol.
class ProofStore {
  public:
    ProofStore(ProofStore&& o) noexcept { *this = std::move(o); }
    ProofStore& operator=(ProofStore&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_; o.h_ = nullptr;
            ctx_ = std::move(o.ctx_); tree_ = std::move(o.tree_);
            height_ = o.height_; aggregation_factor_ = o.aggregation_factor_; policy_ = o.policy_; n_bits_ = o.n_bits_;
        }
        return *this;
    }
    ProofStore(const ProofStore&) = delete;
    ProofStore& operator=(const ProofStore&) = delete;
    ~ProofStore() { reset(); }
    struct Refreshed { uint64_t proved = 0, kept = 0, moved_rows = 0; };
    // every leaf of the tree as it is now
    Refreshed refresh() { return refresh_impl(0, nullptr); }
    // the given leaves, strictly increasing (none: the store is emptied)
    Refreshed refresh(const std::vector<uint64_t>& leaves) {
        static const uint64_t none = 0;
        return refresh_impl(leaves.size(), leaves.empty() ? &none : leaves.data());
    }
    size_t rows() const { return dapol_proof_store_rows(h_); }
    // The stored proof of one leaf; None for a leaf the store does not hold.
    std::optional<DapolProof> proof(uint64_t leaf) const {
        auto v = proofs({leaf});
        return std::move(v[0]);
    }
    std::vector<std::optional<DapolProof>> proofs(const std::vector<uint64_t>& leaves) const {
        const size_t k = leaves.size(), h = (size_t)height_, es = dapol_proof_store_entity_bytes(h_);
        std::vector<uint8_t> found(k + 1, 0), C(k * h * 32 + 1), H(k * h * 32 + 1), R(k * es + 1);
        check(dapol_proof_store_fetch(h_, k, leaves.data(), found.data(), C.data(), H.data(), R.data()));
        std::vector<std::optional<DapolProof>> out(k);
        for (size_t e = 0; e < k; e++) {
            if (!found[e]) continue;
            DapolProof p;
            p.leaf_index = leaves[e];
            p.merkle_siblings.resize(h);
            for (size_t s = 0; s < h; s++) {
                std::memcpy(p.merkle_siblings[s].com.data(), &C[(e * h + s) * 32], 32);
                std::memcpy(p.merkle_siblings[s].hash.data(), &H[(e * h + s) * 32], 32);
            }
            p.range_proofs.assign(R.begin() + e * es, R.begin() + (e + 1) * es);
            p.policy = policy_; p.aggregation_factor = aggregation_factor_; p.n_bits = n_bits_; p.height = height_;
            out[e] = std::move(p);
        }
        return out;
    }
    // DapolProof::verify of every row against the tree as it is now, on the device: true when the store is not empty and every row verifies.
    bool verify() const {
        const size_t n = rows();
        std::vector<uint8_t> ok(n + 1, 0);
        check(dapol_proof_store_verify(h_, nullptr, ok.data()));
        return n > 0 && std::all_of(ok.begin(), ok.begin() + n, [](uint8_t x) { return x != 0; });
    }
  private:
    friend class Dapol;
    ProofStore() = default;
    void reset() { if (h_) dapol_proof_store_destroy(h_); h_ = nullptr; tree_.reset(); ctx_.reset(); }
    Refreshed refresh_impl(size_t b, const uint64_t* idx) {
        Refreshed r;
        check(dapol_proof_store_refresh(h_, b, idx, &r.proved, &r.kept, &r.moved_rows));
        return r;
    }
    dapol_proof_store* h_ = nullptr;
    std::shared_ptr<Context> ctx_;
    std::shared_ptr<dapol_tree> tree_;
    int height_ = 0, n_bits_ = 64;
    size_t aggregation_factor_ = 0;
    Policy policy_ = Policy::Padding;
};

// dapol_batch_store: the proofs of Dapol::generate_proof_batches for one list of batches kept on the GPU and re-proved in place after
// update / insert / remove / apply (Dapol::batch_store makes one).  A row is a batch, in the order of the last refresh.  Move-only; it
// shares ownership of the tree it was made on, as ProofStore does.
class BatchProofStore {
  public:
    BatchProofStore(BatchProofStore&& o) noexcept { *this = std::move(o); }
    BatchProofStore& operator=(BatchProofStore&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_; o.h_ = nullptr;
            ctx_ = std::move(o.ctx_); tree_ = std::move(o.tree_);
            height_ = o.height_; aggregation_factor_ = o.aggregation_factor_; policy_ = o.policy_; n_bits_ = o.n_bits_;
        }
        return *this;
    }
    BatchProofStore(const BatchProofStore&) = delete;
    BatchProofStore& operator=(const BatchProofStore&) = delete;
    ~BatchProofStore() { reset(); }
    struct Refreshed { uint64_t proved = 0, kept = 0, n_calls = 0, moved_rows = 0; };
    // the list the store holds, for the tree as it is now (after update-only edits)
    Refreshed refresh() { return refresh_impl(0, nullptr, nullptr); }
    // another list (none: the store is emptied); a batch whose leaves equal an old row's continues that row.  None when there is no
    // liability at one of the leaves: the store is then as it was.
    std::optional<Refreshed> refresh(const std::vector<std::vector<uint64_t>>& batches) {
        std::vector<uint64_t> boff{0}, idx;
        for (auto& b : batches) { idx.insert(idx.end(), b.begin(), b.end()); boff.push_back(idx.size()); }
        idx.push_back(0);                                             // (never NULL)
        Refreshed r;
        int32_t rc = dapol_batch_store_refresh(h_, batches.size(), boff.data(), idx.data(), &r.proved, &r.kept, &r.n_calls, &r.moved_rows);
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        return r;
    }
    size_t rows() const { return dapol_batch_store_rows(h_); }
    std::vector<std::vector<uint64_t>> batches() const {
        const size_t n = rows();
        std::vector<uint64_t> boff(n + 1);
        check(dapol_batch_store_layout(h_, boff.data(), nullptr, nullptr, nullptr));
        std::vector<uint64_t> idx(boff[n] + 1);
        check(dapol_batch_store_layout(h_, nullptr, idx.data(), nullptr, nullptr));
        std::vector<std::vector<uint64_t>> out(n);
        for (size_t j = 0; j < n; j++) out[j].assign(idx.begin() + boff[j], idx.begin() + boff[j + 1]);
        return out;
    }
    // The stored proofs of the given rows, in any order, duplicates allowed (dapol_batch_store_fetch).
    std::vector<DapolBatchProof> proofs(const std::vector<uint64_t>& rows_wanted) const {
        const size_t n = rows(), k = rows_wanted.size();
        std::vector<uint64_t> boff(n + 1), soff(n + 1), roff(n + 1);
        check(dapol_batch_store_layout(h_, boff.data(), nullptr, soff.data(), roff.data()));
        std::vector<uint64_t> idx(boff[n] + 1);
        check(dapol_batch_store_layout(h_, nullptr, idx.data(), nullptr, nullptr));
        size_t T = 0, R = 0;
        for (uint64_t r : rows_wanted) {
            if (r >= n) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
            T += soff[r + 1] - soff[r]; R += roff[r + 1] - roff[r];
        }
        std::vector<uint8_t> C(T * 32 + 1), H(T * 32 + 1), blob(R + 1);
        check(dapol_batch_store_fetch(h_, k, rows_wanted.data(), C.data(), H.data(), blob.data()));
        std::vector<DapolBatchProof> out(k);
        size_t s0 = 0, r0 = 0;
        for (size_t i = 0; i < k; i++) {
            const size_t r = rows_wanted[i], S = soff[r + 1] - soff[r], B = roff[r + 1] - roff[r];
            DapolBatchProof& p = out[i];
            p.leaf_indexes.assign(idx.begin() + boff[r], idx.begin() + boff[r + 1]);
            p.merkle_siblings.resize(S);
            for (size_t s = 0; s < S; s++) {
                std::memcpy(p.merkle_siblings[s].com.data(), &C[(s0 + s) * 32], 32);
                std::memcpy(p.merkle_siblings[s].hash.data(), &H[(s0 + s) * 32], 32);
            }
            p.range_proofs.assign(blob.begin() + r0, blob.begin() + r0 + B);
            p.policy = policy_; p.aggregation_factor = aggregation_factor_; p.n_bits = n_bits_; p.height = height_;
            s0 += S; r0 += B;
        }
        return out;
    }
    DapolBatchProof proof(uint64_t row) const { return std::move(proofs({row})[0]); }
    // DapolBatchProof::verify_batch of every row against the tree as it is now, on the device (dapol_batch_store_verify).
    std::vector<bool> verdicts() const {
        const size_t n = rows();
        std::vector<uint8_t> ok(n + 1, 0);
        check(dapol_batch_store_verify(h_, nullptr, ok.data()));
        return std::vector<bool>(ok.begin(), ok.begin() + n);
    }
    // true when the store is not empty and every row verifies
    bool verify() const {
        const auto ok = verdicts();
        return !ok.empty() && std::all_of(ok.begin(), ok.end(), [](bool x) { return x; });
    }
  private:
    friend class Dapol;
    BatchProofStore() = default;
    void reset() { if (h_) dapol_batch_store_destroy(h_); h_ = nullptr; tree_.reset(); ctx_.reset(); }
    Refreshed refresh_impl(size_t nb, const uint64_t* boff, const uint64_t* idx) {
        Refreshed r;
        check(dapol_batch_store_refresh(h_, nb, boff, idx, &r.proved, &r.kept, &r.n_calls, &r.moved_rows));
        return r;
    }
    dapol_batch_store* h_ = nullptr;
    std::shared_ptr<Context> ctx_;
    std::shared_ptr<dapol_tree> tree_;
    int height_ = 0, n_bits_ = 64;
    size_t aggregation_factor_ = 0;
    Policy policy_ = Policy::Padding;
};

// Dapol<D, R> (src/dapol/mod.rs:78-83)
class Dapol {
  public:
    // Dapol::new (mod.rs:100-128): validation, leaf derivation (build_leaf_nodes, on the GPU), tree build.  D = the
    // context's digest for node hashes AND leaf derivation, as in the reference.  Throws DapolError with the code of
    // TreeHeightTooBig / SparsityTooSmall / DuplicatedInternalId / FailedToMapIndex.
    static Dapol create(std::shared_ptr<Context> ctx, int digest, const std::vector<Liability>& liabilities, const DapolOptions& options,
                        Policy policy = Policy::Padding) {
        Dapol d = new_blank(std::move(ctx), options.tree_height, options.aggregation_factor, policy);
        const size_t n = liabilities.size();
        const Packed L(liabilities);
        std::vector<uint64_t> idx(n), v(n), by_entity(n);
        std::vector<uint32_t> order(n);
        std::vector<Bytes32> r(n);
        check(dapol_build_leaf_nodes(d.ctx_->get(), digest, options.audit_seed.data(), options.audit_seed.size(), options.tree_height, n, L.iid.data(),
                                     L.ioff.data(), L.eid.data(), L.eoff.data(), L.vals.data(), idx.data(), v.data(), n ? r[0].data() : nullptr,
                                     order.data(), by_entity.data()));
        for (size_t i = 0; i < n; i++) d.id_to_idx_map_[liabilities[i].internal_id] = by_entity[i];
        d.build(idx, v, r, options.secret, true);
        d.digest_ = digest; d.audit_seed_ = options.audit_seed; d.created_ = true;      // what insert_liabilities derives further leaves with
        return d;
    }
    // New liabilities join the tree by id (dapol_tree_insert_liabilities): shuffle_index (mod.rs:408-441) with the tree's current leaves
    // as the indexes already taken, under the digest and the audit seed given to create; then dapol_tree_insert, all or nothing.  With
    // nothing removed since create, ids map where create over the old and the new liabilities would have put them.  An internal id
    // that is in id_to_idx_map() already, or given twice, throws DapolError(DAPOL_ERR_DUPLICATED_INTERNAL_ID) before the library is
    // called (the tree itself holds no ids); the new ids join the map on success only.  A Dapol not made by create has no audit seed:
    // DapolError(DAPOL_ERR_INVALID_ARGUMENT).
    void insert_liabilities(const std::vector<Liability>& liabilities) {
        if (!created_ || !tree_) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        const size_t k = liabilities.size();
        std::map<LiabilityId, uint64_t> fresh;
        for (auto& l : liabilities)
            if (id_to_idx_map_.count(l.internal_id) || !fresh.emplace(l.internal_id, 0).second) throw DapolError(DAPOL_ERR_DUPLICATED_INTERNAL_ID);
        if (k == 0) return;
        const Packed L(liabilities);
        std::vector<uint64_t> by_entity(k);
        check(dapol_tree_insert_liabilities(tree_.get(), digest_, audit_seed_.data(), audit_seed_.size(), k, L.iid.data(), L.ioff.data(), L.eid.data(),
                                            L.eoff.data(), L.vals.data(), by_entity.data()));
        for (size_t i = 0; i < k; i++) id_to_idx_map_[liabilities[i].internal_id] = by_entity[i];
    }
    // Dapol::generate_proof_for_id / generate_proof_batch_for_ids (mod.rs:148-164): None for an unknown id.
    std::optional<DapolProof> generate_proof_for_id(const LiabilityId& id, const Bytes32& nonce_seed, int n_bits = 64) const {
        auto it = id_to_idx_map_.find(id);
        if (it == id_to_idx_map_.end()) return std::nullopt;
        return generate_proof(it->second, nonce_seed, n_bits);
    }
    std::optional<DapolBatchProof> generate_proof_batch_for_ids(const std::vector<LiabilityId>& ids, const Bytes32& nonce_seed, int n_bits = 64) const {
        std::vector<uint64_t> idx;
        for (auto& id : ids) {
            auto it = id_to_idx_map_.find(id);
            if (it == id_to_idx_map_.end()) return std::nullopt;
            idx.push_back(it->second);
        }
        return generate_proof_batch(idx, nonce_seed, n_bits);
    }
    // generate_proof_batch_for_ids for many lists of ids in one call (generate_proof_batches): None when one id is unknown.
    std::optional<std::vector<DapolBatchProof>> generate_proof_batches_for_ids(const std::vector<std::vector<LiabilityId>>& ids, const Bytes32& nonce_seed,
                                                                               int n_bits = 64) const {
        std::vector<std::vector<uint64_t>> batches(ids.size());
        for (size_t j = 0; j < ids.size(); j++)
            for (auto& id : ids[j]) {
                auto it = id_to_idx_map_.find(id);
                if (it == id_to_idx_map_.end()) return std::nullopt;
                batches[j].push_back(it->second);
            }
        return generate_proof_batches(batches, nonce_seed, n_bits);
    }
    const std::map<LiabilityId, uint64_t>& id_to_idx_map() const { return id_to_idx_map_; }
    // Dapol::new_blank (mod.rs:196-204)
    static Dapol new_blank(std::shared_ptr<Context> ctx, int height, size_t aggregation_factor, Policy policy = Policy::Padding) {
        Dapol d;
        d.ctx_ = std::move(ctx);
        d.height_ = height;
        d.aggregation_factor_ = aggregation_factor;
        d.policy_ = policy;
        return d;
    }
    // Dapol::build (mod.rs:206-208): input = sorted (tree index, value, blinding); pad_seed stands in for thread_rng().
    void build(const std::vector<uint64_t>& idx, const std::vector<uint64_t>& values, const std::vector<Bytes32>& blindings,
               const Bytes32& pad_seed, bool enforce_sparsity = false) {
        if (idx.size() != values.size() || idx.size() != blindings.size()) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        dapol_tree* t = nullptr;
        check(dapol_tree_build(ctx_->get(), height_, idx.size(), idx.data(), values.data(), blindings.empty() ? nullptr : blindings[0].data(),
                               pad_seed.data(), enforce_sparsity ? 1 : 0, &t));
        tree_.reset(t, [](dapol_tree* p) { dapol_tree_destroy(p); });
    }
    // Dapol::update (mod.rs:211-213): inserts the liability at idx or replaces the one already there.  On a blank
    // Dapol the first update creates the tree with pad_seed; later calls ignore pad_seed (a tree has one seed).  Without a
    // seed a blank Dapol draws one from the OS (the reference draws every padding blinding from thread_rng, node.rs:87).
    void update(uint64_t idx, uint64_t value, const Bytes32& blinding) { update(idx, value, blinding, tree_ ? Bytes32{} : get_secret()); }
    void update(uint64_t idx, uint64_t value, const Bytes32& blinding, const Bytes32& pad_seed) {
        if (!tree_) return build({idx}, {value}, {blinding}, pad_seed);
        check(dapol_tree_update(tree_.get(), 1, &idx, &value, blinding.data()));
    }
    // The batched form: k updates applied in order by one level-parallel rebuild.
    void update(const std::vector<uint64_t>& idx, const std::vector<uint64_t>& values, const std::vector<Bytes32>& blindings) {
        update(idx, values, blindings, tree_ ? Bytes32{} : get_secret());
    }
    void update(const std::vector<uint64_t>& idx, const std::vector<uint64_t>& values, const std::vector<Bytes32>& blindings,
                const Bytes32& pad_seed) {
        if (idx.size() != values.size() || idx.size() != blindings.size()) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        if (idx.empty()) return;
        if (!tree_) {
            update(idx[0], values[0], blindings[0], pad_seed);
            if (idx.size() > 1) check(dapol_tree_update(tree_.get(), idx.size() - 1, idx.data() + 1, values.data() + 1, blindings[1].data()));
            return;
        }
        check(dapol_tree_update(tree_.get(), idx.size(), idx.data(), values.data(), blindings[0].data()));
    }
    // Adds NEW liabilities at these leaf indexes (dapol_tree_insert; in any order, all or nothing): the tree equals a build over the old
    // and the new leaves with the same seed.  An index that is a leaf already (or given twice) throws
    // DapolError(DAPOL_ERR_INVALID_ARGUMENT) with nothing inserted.  On a blank Dapol it builds over the whole batch (sorted here; all or nothing too).  By liability
    // id: insert_liabilities.
    void insert(const std::vector<uint64_t>& idx, const std::vector<uint64_t>& values, const std::vector<Bytes32>& blindings) {
        insert(idx, values, blindings, tree_ ? Bytes32{} : get_secret());
    }
    void insert(const std::vector<uint64_t>& idx, const std::vector<uint64_t>& values, const std::vector<Bytes32>& blindings, const Bytes32& pad_seed) {
        if (idx.size() != values.size() || idx.size() != blindings.size()) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        if (idx.empty()) return;
        if (tree_) return check(dapol_tree_insert(tree_.get(), idx.size(), idx.data(), values.data(), blindings[0].data()));
        std::vector<size_t> ord(idx.size());                         // a blank Dapol: one build over the whole batch, all or nothing as well
        for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
        std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return idx[a] < idx[b]; });
        std::vector<uint64_t> si, sv;
        std::vector<Bytes32> sr;
        for (size_t b = 0; b < ord.size(); b++) {
            if (b && idx[ord[b]] == idx[ord[b - 1]]) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
            si.push_back(idx[ord[b]]); sv.push_back(values[ord[b]]); sr.push_back(blindings[ord[b]]);
        }
        build(si, sv, sr, pad_seed);
    }
    // Removes the liabilities at these leaf indexes (dapol_tree_remove; the crate has no removal): all or nothing, the survivors keep
    // their indexes, and the tree equals a build over the survivors with the same seed.  An index that is not a leaf throws
    // DapolError(DAPOL_ERR_UNKNOWN_LEAF); removing every leaf throws DapolError(DAPOL_ERR_INVALID_ARGUMENT).
    void remove(const std::vector<uint64_t>& idx) {
        if (idx.empty()) return;
        if (!tree_) throw DapolError(DAPOL_ERR_UNKNOWN_LEAF);
        check(dapol_tree_remove(tree_.get(), idx.size(), idx.data()));
    }
    // The same by internal id; the ids leave id_to_idx_map() too.  An unknown id throws DapolError(DAPOL_ERR_UNKNOWN_LEAF) with
    // nothing removed.
    void remove_ids(const std::vector<LiabilityId>& ids) {
        std::vector<uint64_t> idx;
        for (auto& id : ids) {
            auto it = id_to_idx_map_.find(id);
            if (it == id_to_idx_map_.end()) throw DapolError(DAPOL_ERR_UNKNOWN_LEAF);
            idx.push_back(it->second);
        }
        remove(idx);
        for (auto& id : ids) id_to_idx_map_.erase(id);
    }
    // A mixed change set as ONE edit (dapol_tree_apply; all or nothing): the liabilities at `remove` go, a put replaces the liability
    // at its index or adds one, and the tree equals a build over the resulting leaves with the same seed.  Returns, per put, whether
    // it added a leaf.  Throws with nothing applied: DapolError(DAPOL_ERR_INVALID_ARGUMENT) for an index twice among the puts, an
    // index both removed and put, or a result with no leaf; DapolError(DAPOL_ERR_UNKNOWN_LEAF) for a removal that is not a leaf.
    // Where three calls to remove / insert / update would leave the first ones applied when a later one is refused, this leaves none.
    std::vector<bool> apply(const std::vector<uint64_t>& remove, const std::vector<uint64_t>& put_idx, const std::vector<uint64_t>& values,
                            const std::vector<Bytes32>& blindings) {
        if (put_idx.size() != values.size() || put_idx.size() != blindings.size()) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        if (remove.empty() && put_idx.empty()) return {};
        if (!tree_) throw DapolError(remove.empty() ? DAPOL_ERR_INVALID_ARGUMENT : DAPOL_ERR_UNKNOWN_LEAF);      // (a blank Dapol: build or insert)
        std::vector<uint8_t> was_new(put_idx.size() + 1);
        check(dapol_tree_apply(tree_.get(), remove.size(), remove.data(), put_idx.size(), put_idx.data(), values.data(),
                               blindings.empty() ? nullptr : blindings[0].data(), was_new.data()));
        return std::vector<bool>(was_new.begin(), was_new.end() - 1);
    }
    // The same by internal id, for a Dapol made by create: the liabilities of remove_ids go and `liabilities` join in one edit.  The new
    // indexes are derived as insert_liabilities derives them (dapol_tree_derive_leaves: the tree's current leaves count as taken, those
    // that go in this very call included).  An unknown id to remove throws DapolError(DAPOL_ERR_UNKNOWN_LEAF); a new internal id that is
    // in id_to_idx_map() already -- also one that is being removed -- or given twice throws DapolError(DAPOL_ERR_DUPLICATED_INTERNAL_ID);
    // both before the library is called.  id_to_idx_map() changes only when the library call has succeeded.
    void apply_liabilities(const std::vector<LiabilityId>& remove_ids, const std::vector<Liability>& liabilities) {
        if (!created_ || !tree_) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        std::vector<uint64_t> gone;
        for (auto& id : remove_ids) {
            auto it = id_to_idx_map_.find(id);
            if (it == id_to_idx_map_.end()) throw DapolError(DAPOL_ERR_UNKNOWN_LEAF);
            gone.push_back(it->second);
        }
        const size_t k = liabilities.size();
        std::map<LiabilityId, uint64_t> fresh;
        for (auto& l : liabilities)
            if (id_to_idx_map_.count(l.internal_id) || !fresh.emplace(l.internal_id, 0).second) throw DapolError(DAPOL_ERR_DUPLICATED_INTERNAL_ID);
        if (gone.empty() && k == 0) return;
        std::vector<uint64_t> idx(k), v(k), by_entity(k);
        std::vector<Bytes32> r(k);
        std::vector<uint32_t> order(k);
        if (k) {
            const Packed L(liabilities);
            check(dapol_tree_derive_leaves(tree_.get(), digest_, audit_seed_.data(), audit_seed_.size(), k, L.iid.data(), L.ioff.data(), L.eid.data(),
                                           L.eoff.data(), L.vals.data(), idx.data(), v.data(), r[0].data(), order.data(), by_entity.data()));
        }
        check(dapol_tree_apply(tree_.get(), gone.size(), gone.data(), k, idx.data(), v.data(), k ? r[0].data() : nullptr, nullptr));
        for (auto& id : remove_ids) id_to_idx_map_.erase(id);
        for (size_t i = 0; i < k; i++) id_to_idx_map_[liabilities[i].internal_id] = by_entity[i];
    }
    // Dapol::root_raw / Dapol::root (mod.rs:134-141)
    DapolNode root_raw() const {
        DapolNode n;
        check(dapol_tree_root(tree_.get(), n.com.data(), n.hash.data(), &n.v, n.v_blinding.data()));
        return n;
    }
    DapolProofNode root() const { return root_raw().get_proof_node(); }
    // Dapol::generate_proof (mod.rs:167-169): None when there is no liability at the leaf.
    std::optional<DapolProof> generate_proof(uint64_t leaf_idx, const Bytes32& nonce_seed, int n_bits = 64) const {
        auto v = generate_proofs({leaf_idx}, nonce_seed, n_bits);
        if (!v) return std::nullopt;
        return std::move((*v)[0]);
    }
    // Dapol::generate_proof_batch (mod.rs:172-190): ONE proof for all the leaves (strictly increasing indexes); None
    // when there is no liability at one of them.
    std::optional<DapolBatchProof> generate_proof_batch(const std::vector<uint64_t>& leaves, const Bytes32& nonce_seed, int n_bits = 64) const {
        size_t S = 0;
        check(dapol_batch_siblings(height_, leaves.size(), leaves.data(), &S, nullptr, nullptr));
        size_t es = dapol_entity_proof_size((int)S, (int)policy_, (int)aggregation_factor_, n_bits);
        if (es == 0) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        std::vector<uint8_t> C(S * 32 + 1), H(S * 32 + 1);
        DapolBatchProof out;
        out.range_proofs.resize(es);
        int32_t rc = dapol_prove_batch(ctx_->get(), tree_.get(), leaves.size(), leaves.data(), (int)policy_, (int)aggregation_factor_, n_bits,
                                       nonce_seed.data(), C.data(), H.data(), out.range_proofs.data());
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        out.leaf_indexes = leaves;
        out.merkle_siblings.resize(S);
        for (size_t s = 0; s < S; s++) {
            std::memcpy(out.merkle_siblings[s].com.data(), &C[s * 32], 32);
            std::memcpy(out.merkle_siblings[s].hash.data(), &H[s * 32], 32);
        }
        out.policy = policy_; out.aggregation_factor = aggregation_factor_; out.n_bits = n_bits; out.height = height_;
        return out;
    }
    // generate_proof_batch for MANY lists of leaves in one GPU call (dapol_prove_batches): out[j] equals generate_proof_batch(batches[j])
    // under the same seed, byte for byte; batches may overlap and repeat.  None when there is no liability at one of the leaves.
    std::optional<std::vector<DapolBatchProof>> generate_proof_batches(const std::vector<std::vector<uint64_t>>& batches, const Bytes32& nonce_seed,
                                                                       int n_bits = 64) const {
        const size_t nb = batches.size();
        std::vector<uint64_t> boff{0}, idx;
        for (auto& b : batches) { idx.insert(idx.end(), b.begin(), b.end()); boff.push_back(idx.size()); }
        idx.push_back(0);                                             // (never NULL)
        std::vector<uint64_t> soff(nb + 1), roff(nb + 1);
        check(dapol_batches_plan(height_, nb, boff.data(), idx.data(), (int)policy_, (int)aggregation_factor_, n_bits, nullptr, soff.data(), roff.data(), nullptr));
        std::vector<uint8_t> C(soff[nb] * 32 + 1), H(soff[nb] * 32 + 1), blob(roff[nb] + 1);
        int32_t rc = dapol_prove_batches(ctx_->get(), tree_.get(), nb, boff.data(), idx.data(), (int)policy_, (int)aggregation_factor_, n_bits, nonce_seed.data(),
                                         C.data(), H.data(), blob.data(), nullptr);
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        std::vector<DapolBatchProof> out(nb);
        for (size_t j = 0; j < nb; j++) {
            DapolBatchProof& p = out[j];
            p.leaf_indexes = batches[j];
            p.merkle_siblings.resize(soff[j + 1] - soff[j]);
            for (size_t s = 0; s < p.merkle_siblings.size(); s++) {
                std::memcpy(p.merkle_siblings[s].com.data(), &C[(soff[j] + s) * 32], 32);
                std::memcpy(p.merkle_siblings[s].hash.data(), &H[(soff[j] + s) * 32], 32);
            }
            p.range_proofs.assign(blob.begin() + roff[j], blob.begin() + roff[j + 1]);
            p.policy = policy_; p.aggregation_factor = aggregation_factor_; p.n_bits = n_bits; p.height = height_;
        }
        return out;
    }
    // After update / insert / remove / apply: generate_proof_batches' proofs for the tree as it is now, proving only the sub-proofs whose
    // sibling commitments moved (dapol_reprove_batches) and keeping the bytes of the others.  out[j] is the proof for
    // old_proofs[j].leaf_indexes: the caller drops the proofs of batches that lost a leaf, and passes a DapolBatchProof with only its
    // leaf_indexes set for a batch that is new -- an old proof that is not of this Dapol's shape (height, policy, aggregation factor,
    // n_bits, sibling count, blob length) is proved from scratch.  Returns the proofs and the number of range proofs actually computed;
    // None when there is no liability at one of the leaves.  With old proofs from generate_proof_batches (or generate_proof_batch)
    // under the same nonce_seed the result equals generate_proof_batches' byte for byte.  Old bytes are not checked:
    // DapolBatchProof::verify_batch is the check.
    std::optional<std::pair<std::vector<DapolBatchProof>, uint64_t>> regenerate_proof_batches(const std::vector<DapolBatchProof>& old_proofs,
                                                                                             const Bytes32& nonce_seed, int n_bits = 64) const {
        const size_t nb = old_proofs.size();
        std::vector<uint64_t> boff{0}, idx;
        for (auto& p : old_proofs) { idx.insert(idx.end(), p.leaf_indexes.begin(), p.leaf_indexes.end()); boff.push_back(idx.size()); }
        idx.push_back(0);                                             // (never NULL)
        std::vector<uint64_t> soff(nb + 1), roff(nb + 1);
        check(dapol_batches_plan(height_, nb, boff.data(), idx.data(), (int)policy_, (int)aggregation_factor_, n_bits, nullptr, soff.data(), roff.data(), nullptr));
        std::vector<uint8_t> has_old(nb + 1, 0), oldC(soff[nb] * 32 + 1, 0), oldR(roff[nb] + 1, 0), C(soff[nb] * 32 + 1), H(soff[nb] * 32 + 1), blob(roff[nb] + 1);
        for (size_t j = 0; j < nb; j++) {
            const DapolBatchProof& p = old_proofs[j];
            if (p.height != height_ || p.policy != policy_ || p.aggregation_factor != aggregation_factor_ || p.n_bits != n_bits ||
                p.merkle_siblings.size() != soff[j + 1] - soff[j] || p.range_proofs.size() != roff[j + 1] - roff[j])
                continue;
            has_old[j] = 1;
            for (size_t s = 0; s < p.merkle_siblings.size(); s++) std::memcpy(&oldC[(soff[j] + s) * 32], p.merkle_siblings[s].com.data(), 32);
            if (!p.range_proofs.empty()) std::memcpy(&oldR[roff[j]], p.range_proofs.data(), p.range_proofs.size());
        }
        uint64_t proved = 0;
        int32_t rc = dapol_reprove_batches(ctx_->get(), tree_.get(), nb, boff.data(), idx.data(), (int)policy_, (int)aggregation_factor_, n_bits, nonce_seed.data(),
                                           has_old.data(), oldC.data(), oldR.data(), C.data(), H.data(), blob.data(), &proved, nullptr, nullptr);
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        std::vector<DapolBatchProof> out(nb);
        for (size_t j = 0; j < nb; j++) {
            DapolBatchProof& p = out[j];
            p.leaf_indexes = old_proofs[j].leaf_indexes;
            p.merkle_siblings.resize(soff[j + 1] - soff[j]);
            for (size_t s = 0; s < p.merkle_siblings.size(); s++) {
                std::memcpy(p.merkle_siblings[s].com.data(), &C[(soff[j] + s) * 32], 32);
                std::memcpy(p.merkle_siblings[s].hash.data(), &H[(soff[j] + s) * 32], 32);
            }
            p.range_proofs.assign(blob.begin() + roff[j], blob.begin() + roff[j + 1]);
            p.policy = policy_; p.aggregation_factor = aggregation_factor_; p.n_bits = n_bits; p.height = height_;
        }
        return std::make_pair(std::move(out), proved);
    }
    // What regenerate_proof_batches would prove after the leaves `edited` (strictly increasing: replaced, inserted and removed ones)
    // changed, without a GPU call (dapol_reprove_batches_plan).  has_old: empty = every batch has an old proof, else one flag per batch.
    struct BatchesReprovePlan {
        std::vector<uint64_t> proved_per_batch;          // dirty sub-proofs of each batch
        uint64_t proved = 0, sum_m_proved = 0, sum_m_all = 0;
    };
    BatchesReprovePlan regenerate_proof_batches_plan(const std::vector<std::vector<uint64_t>>& batches, const std::vector<uint64_t>& edited,
                                                     const std::vector<uint8_t>& has_old = {}, int n_bits = 64) const {
        const size_t nb = batches.size();
        if (!has_old.empty() && has_old.size() != nb) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        std::vector<uint64_t> boff{0}, idx;
        for (auto& b : batches) { idx.insert(idx.end(), b.begin(), b.end()); boff.push_back(idx.size()); }
        idx.push_back(0);                                             // (never NULL)
        BatchesReprovePlan out;
        out.proved_per_batch.assign(nb + 1, 0);
        check(dapol_reprove_batches_plan(height_, nb, boff.data(), idx.data(), has_old.empty() ? nullptr : has_old.data(), edited.size(), edited.data(),
                                         (int)policy_, (int)aggregation_factor_, n_bits, out.proved_per_batch.data(), &out.proved, &out.sum_m_proved, &out.sum_m_all));
        out.proved_per_batch.resize(nb);
        return out;
    }
    // Many single-leaf proofs in one GPU batch (the throughput path).
    std::optional<std::vector<DapolProof>> generate_proofs(const std::vector<uint64_t>& leaves, const Bytes32& nonce_seed, int n_bits = 64) const {
        return prove_many(leaves, nonce_seed, n_bits, false);
    }
    // The same proofs with every distinct sub-proof statement proven once (dapol_prove_entities_shared; the crate's
    // generate_all_proofs DFS, mod.rs:216-314): strictly increasing leaves, same layout, verified and serialised like
    // generate_proofs' -- only the nonce streams differ (keyed by the subtree a sub-proof speaks about, not by the leaf).
    std::optional<std::vector<DapolProof>> generate_proofs_shared(const std::vector<uint64_t>& leaves, const Bytes32& nonce_seed, int n_bits = 64) const {
        return prove_many(leaves, nonce_seed, n_bits, true);
    }
    // After update / insert / remove: generate_proofs_shared's proofs for the tree as it is now, proving only the sub-proofs whose
    // sibling commitments moved (dapol_reprove_entities_shared) and keeping the bytes of the others from old_proofs, which are matched
    // to `leaves` (strictly increasing) by leaf_index; a leaf without an old proof of this Dapol's shape is proved from scratch, old
    // proofs of leaves that are gone are ignored.  Returns the proofs and the number of range proofs actually computed.  With old
    // proofs from generate_proofs_shared under the same nonce_seed the result equals generate_proofs_shared's byte for byte.  Old bytes
    // are not checked: DapolProof::verify is the check.
    std::optional<std::pair<std::vector<DapolProof>, uint64_t>> regenerate_proofs_shared(const std::vector<uint64_t>& leaves, const std::vector<DapolProof>& old_proofs,
                                                                                         const Bytes32& nonce_seed, int n_bits = 64) const {
        const size_t es = dapol_entity_proof_size(height_, (int)policy_, (int)aggregation_factor_, n_bits);
        if (es == 0) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        const size_t b = leaves.size(), h = (size_t)height_;
        std::map<uint64_t, const DapolProof*> by_leaf;
        for (auto& p : old_proofs)
            if (p.height == height_ && p.policy == policy_ && p.aggregation_factor == aggregation_factor_ && p.n_bits == n_bits && p.merkle_siblings.size() == h &&
                p.range_proofs.size() == es)
                by_leaf[p.leaf_index] = &p;
        std::vector<uint8_t> has_old(b + 1, 0), oldC(b * h * 32 + 1, 0), oldR(b * es + 1, 0), C(b * h * 32 + 1), H(b * h * 32 + 1), R(b * es + 1);
        for (size_t e = 0; e < b; e++) {
            auto it = by_leaf.find(leaves[e]);
            if (it == by_leaf.end()) continue;
            has_old[e] = 1;
            for (size_t s = 0; s < h; s++) std::memcpy(&oldC[(e * h + s) * 32], it->second->merkle_siblings[s].com.data(), 32);
            std::memcpy(&oldR[e * es], it->second->range_proofs.data(), es);
        }
        uint64_t proved = 0;
        int32_t rc = dapol_reprove_entities_shared(ctx_->get(), tree_.get(), b, leaves.data(), (int)policy_, (int)aggregation_factor_, n_bits, nonce_seed.data(),
                                                   has_old.data(), oldC.data(), oldR.data(), C.data(), H.data(), R.data(), &proved, nullptr);
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        return std::make_pair(unpack(leaves, C, H, R, es, n_bits), proved);
    }
    // An empty device-resident store of this tree's shared proofs under nonce_seed (dapol_proof_store_create): refresh() fills it and
    // brings it up to date after edits, proof(leaf) serves from it.  The tree must have been built.
    ProofStore proof_store(const Bytes32& nonce_seed, int n_bits = 64) const {
        ProofStore st;
        check(dapol_proof_store_create(ctx_->get(), tree_.get(), (int)policy_, (int)aggregation_factor_, n_bits, nonce_seed.data(), &st.h_));
        st.ctx_ = ctx_; st.tree_ = tree_;
        st.height_ = height_; st.aggregation_factor_ = aggregation_factor_; st.policy_ = policy_; st.n_bits_ = n_bits;
        return st;
    }
    // An empty device-resident store of this tree's batch proofs under nonce_seed (dapol_batch_store_create): refresh(batches) fills it,
    // refresh() brings it up to date after edits, proof(row) serves from it.  The tree must have been built.
    BatchProofStore batch_store(const Bytes32& nonce_seed, int n_bits = 64) const {
        BatchProofStore st;
        check(dapol_batch_store_create(ctx_->get(), tree_.get(), (int)policy_, (int)aggregation_factor_, n_bits, nonce_seed.data(), &st.h_));
        st.ctx_ = ctx_; st.tree_ = tree_;
        st.height_ = height_; st.aggregation_factor_ = aggregation_factor_; st.policy_ = policy_; st.n_bits_ = n_bits;
        return st;
    }
    // Verifies many single-leaf proofs in one call with every run of equal sub-proofs checked once (dapol_verify_entities_shared):
    // a verdict per proof -- the ones DapolProof::verify gives one by one -- and the number of range proofs actually checked.  Proofs
    // of generate_proofs_shared in their order share the most; any proofs of one (height, policy, aggregation factor, n_bits) may
    // be passed.  proofs[i] is checked against leaves[i].
    static std::pair<std::vector<bool>, uint64_t> verify_proofs_shared(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves,
                                                                       const std::vector<DapolProof>& proofs) {
        return verify_many_shared(ctx, root, leaves, proofs, nullptr);
    }
    static std::pair<std::vector<bool>, uint64_t> verify_proofs_shared(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves,
                                                                       const std::vector<DapolProof>& proofs, const Bytes32& verify_seed) {
        return verify_many_shared(ctx, root, leaves, proofs, verify_seed.data());
    }
    // The COMPACT form of generate_proofs_shared (dapol_prove_entities_shared_compact): the Merkle paths per leaf and every distinct
    // sub-proof once -- what leaves the GPU and what verify_proofs_compact takes.  expand() cuts the proofs of single leaves out.
    struct CompactProofs {
        std::vector<uint64_t> leaves;                    // strictly increasing
        std::vector<std::vector<DapolProofNode>> merkle_siblings;       // [leaf][height]
        std::vector<uint8_t> compact;                    // the layout of dapol_shared_compact_plan over `leaves`
        uint64_t unique = 0;                             // range proofs actually computed
        Policy policy = Policy::Padding;
        size_t aggregation_factor = 0;
        int n_bits = 64, height = 0;
        // proofs [first, first + count) as generate_proofs_shared returns them (count = 1: one user's proof)
        std::vector<DapolProof> expand(size_t first, size_t count) const {
            const size_t es = dapol_entity_proof_size(height, (int)policy, (int)aggregation_factor, n_bits);
            std::vector<uint8_t> R(count * es + 1);
            check(dapol_shared_expand(height, leaves.size(), leaves.data(), (int)policy, (int)aggregation_factor, n_bits, compact.data(), compact.size(), first, count,
                                      R.data()));
            std::vector<DapolProof> out(count);
            for (size_t i = 0; i < count; i++) {
                out[i].leaf_index = leaves[first + i];
                out[i].merkle_siblings = merkle_siblings[first + i];
                out[i].range_proofs.assign(R.begin() + i * es, R.begin() + (i + 1) * es);
                out[i].policy = policy; out[i].aggregation_factor = aggregation_factor; out[i].n_bits = n_bits; out[i].height = height;
            }
            return out;
        }
        std::vector<DapolProof> expand() const { return expand(0, leaves.size()); }
    };
    std::optional<CompactProofs> generate_proofs_compact(const std::vector<uint64_t>& leaves, const Bytes32& nonce_seed, int n_bits = 64) const {
        const size_t b = leaves.size(), h = (size_t)height_;
        uint64_t len = 0;
        check(dapol_shared_compact_plan(height_, b, leaves.data(), (int)policy_, (int)aggregation_factor_, n_bits, nullptr, nullptr, &len));
        CompactProofs out;
        std::vector<uint8_t> C(b * h * 32 + 1), H(b * h * 32 + 1);
        out.compact.resize((size_t)len + 1);                                 // never pass a null data pointer
        int32_t rc = dapol_prove_entities_shared_compact(ctx_->get(), tree_.get(), b, leaves.data(), (int)policy_, (int)aggregation_factor_, n_bits, nonce_seed.data(),
                                                         0, nullptr, nullptr, nullptr, nullptr, C.data(), H.data(), out.compact.data(), (size_t)len, &len, &out.unique);
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        out.compact.resize((size_t)len);
        out.leaves = leaves;
        out.merkle_siblings.assign(b, std::vector<DapolProofNode>(h));
        for (size_t e = 0; e < b; e++)
            for (size_t s = 0; s < h; s++) {
                std::memcpy(out.merkle_siblings[e][s].com.data(), &C[(e * h + s) * 32], 32);
                std::memcpy(out.merkle_siblings[e][s].hash.data(), &H[(e * h + s) * 32], 32);
            }
        out.policy = policy_; out.aggregation_factor = aggregation_factor_; out.n_bits = n_bits; out.height = height_;
        return out;
    }
    // dapol_verify_entities_compact: the verdicts DapolProof::verify gives for proofs.expand() one by one, with every distinct sub-proof
    // uploaded and checked once, and the number of range proofs actually checked.  proofs.leaves[i] is checked against leaves[i].
    static std::pair<std::vector<bool>, uint64_t> verify_proofs_compact(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves,
                                                                        const CompactProofs& proofs, const uint8_t* verify_seed32 = nullptr) {
        const size_t b = proofs.leaves.size();
        if (leaves.size() != b || proofs.merkle_siblings.size() != b) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        std::vector<bool> out(b, false);
        if (b == 0) return {out, 0};
        std::vector<uint8_t> lC(b * 32), lH(b * 32), C, H, R(proofs.compact);
        for (size_t e = 0; e < b; e++) {
            std::memcpy(&lC[e * 32], leaves[e].com.data(), 32);
            std::memcpy(&lH[e * 32], leaves[e].hash.data(), 32);
            for (auto& s : proofs.merkle_siblings[e]) { C.insert(C.end(), s.com.begin(), s.com.end()); H.insert(H.end(), s.hash.begin(), s.hash.end()); }
        }
        const size_t n_nodes = C.size() / 32, r_len = R.size();
        C.push_back(0); H.push_back(0); R.push_back(0);                     // never pass a null data pointer
        std::vector<uint8_t> ok(b, 0);
        uint64_t unique = 0;
        check(dapol_verify_entities_compact(ctx.get(), proofs.height, b, proofs.leaves.data(), lC.data(), lH.data(), n_nodes, C.data(), H.data(), root.com.data(),
                                            root.hash.data(), (int)proofs.policy, (int)proofs.aggregation_factor, proofs.n_bits, R.data(), r_len, verify_seed32,
                                            ok.data(), &unique));
        for (size_t e = 0; e < b; e++) out[e] = ok[e] != 0;
        return {out, unique};
    }
    // COMPACT Merkle paths (dapol_tree_paths_compact): every distinct sibling of the paths of `leaves` once, root side first, in the
    // layout of dapol_compact_paths_plan -- what verify_proofs_compact_paths takes.  expand() cuts the paths of single leaves out.
    struct CompactPaths {
        std::vector<uint64_t> leaves;                    // strictly increasing
        std::vector<uint8_t> com, hash;                  // [records][32] each
        int height = 0;
        size_t records() const { return com.size() / 32; }
        // the siblings of rows [first, first + count) as generate_proof returns them (count = 1: one user's path)
        std::vector<std::vector<DapolProofNode>> expand(size_t first, size_t count) const {
            const size_t h = (size_t)height;
            std::vector<uint8_t> C(count * h * 32 + 1), H(count * h * 32 + 1);
            std::vector<uint8_t> cC(com), cH(hash);
            cC.push_back(0); cH.push_back(0);                                 // never pass a null data pointer
            check(dapol_compact_paths_expand(32, height, leaves.size(), leaves.data(), cC.data(), cH.data(), records(), first, count, C.data(), H.data()));
            std::vector<std::vector<DapolProofNode>> out(count, std::vector<DapolProofNode>(h));
            for (size_t e = 0; e < count; e++)
                for (size_t s = 0; s < h; s++) {
                    std::memcpy(out[e][s].com.data(), &C[(e * h + s) * 32], 32);
                    std::memcpy(out[e][s].hash.data(), &H[(e * h + s) * 32], 32);
                }
            return out;
        }
        std::vector<std::vector<DapolProofNode>> expand() const { return expand(0, leaves.size()); }
    };
    // nullopt: no liability at one of the leaves.  Plain trees (no upper siblings).
    std::optional<CompactPaths> generate_paths_compact(const std::vector<uint64_t>& leaves) const {
        const size_t b = leaves.size();
        uint64_t n = 0;
        if (dapol_compact_paths_plan(height_, b, leaves.data(), nullptr, nullptr, &n) != DAPOL_OK) n = 0;      // (the call below says what is wrong with the leaves)
        int32_t rc;
        CompactPaths out;
        out.com.resize((size_t)n * 32 + 1); out.hash.resize((size_t)n * 32 + 1);
        rc = dapol_tree_paths_compact(tree_.get(), b, leaves.data(), out.com.data(), out.hash.data(), (size_t)n, &n);
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        out.com.resize((size_t)n * 32); out.hash.resize((size_t)n * 32);
        out.leaves = leaves;
        out.height = height_;
        return out;
    }
    // dapol_verify_entities_compact_paths: verify_proofs_compact's verdicts with paths.expand() as the Merkle siblings (those of `proofs`
    // are not read), every distinct node of the paths merged once.  Returns the verdicts, the range proofs actually checked and the
    // merges made (paths.records() when sharing answered the call).
    struct CompactPathsVerdict { std::vector<bool> ok; uint64_t unique = 0, path_merges = 0; };
    static CompactPathsVerdict verify_proofs_compact_paths(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves,
                                                           const CompactProofs& proofs, const CompactPaths& paths, const uint8_t* verify_seed32 = nullptr) {
        const size_t b = proofs.leaves.size();
        if (leaves.size() != b || paths.leaves != proofs.leaves || paths.height != proofs.height || paths.hash.size() != paths.com.size())
            throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        CompactPathsVerdict out;
        out.ok.assign(b, false);
        if (b == 0) return out;
        std::vector<uint8_t> lC(b * 32), lH(b * 32), C(paths.com), H(paths.hash), R(proofs.compact);
        for (size_t e = 0; e < b; e++) {
            std::memcpy(&lC[e * 32], leaves[e].com.data(), 32);
            std::memcpy(&lH[e * 32], leaves[e].hash.data(), 32);
        }
        const size_t r_len = R.size();
        C.push_back(0); H.push_back(0); R.push_back(0);                     // never pass a null data pointer
        std::vector<uint8_t> ok(b, 0);
        check(dapol_verify_entities_compact_paths(ctx.get(), proofs.height, b, proofs.leaves.data(), lC.data(), lH.data(), paths.records(), C.data(), H.data(),
                                                  root.com.data(), root.hash.data(), (int)proofs.policy, (int)proofs.aggregation_factor, proofs.n_bits, R.data(),
                                                  r_len, verify_seed32, ok.data(), &out.unique, &out.path_merges));
        for (size_t e = 0; e < b; e++) out.ok[e] = ok[e] != 0;
        return out;
    }
  private:
    static std::pair<std::vector<bool>, uint64_t> verify_many_shared(const Context& ctx, const DapolProofNode& root, const std::vector<DapolProofNode>& leaves,
                                                                     const std::vector<DapolProof>& proofs, const uint8_t* verify_seed) {
        const size_t b = proofs.size();
        if (leaves.size() != b) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        std::vector<bool> out(b, false);
        if (b == 0) return {out, 0};
        const DapolProof& p0 = proofs[0];
        std::vector<uint64_t> idx(b);
        std::vector<uint8_t> lC(b * 32), lH(b * 32), C, H, R;
        for (size_t e = 0; e < b; e++) {
            const DapolProof& p = proofs[e];
            if (p.height != p0.height || p.policy != p0.policy || p.aggregation_factor != p0.aggregation_factor || p.n_bits != p0.n_bits)
                throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
            idx[e] = p.leaf_index;
            std::memcpy(&lC[e * 32], leaves[e].com.data(), 32);
            std::memcpy(&lH[e * 32], leaves[e].hash.data(), 32);
            for (auto& s : p.merkle_siblings) { C.insert(C.end(), s.com.begin(), s.com.end()); H.insert(H.end(), s.hash.begin(), s.hash.end()); }
            R.insert(R.end(), p.range_proofs.begin(), p.range_proofs.end());
        }
        const size_t n_nodes = C.size() / 32, r_len = R.size();
        C.push_back(0); H.push_back(0); R.push_back(0);                     // never pass a null data pointer
        std::vector<uint8_t> ok(b, 0);
        uint64_t unique = 0;
        // the length-checked entry point: proofs whose sibling counts or range-proof bytes do not add up are simply invalid
        check(dapol_verify_entities_shared(ctx.get(), p0.height, b, idx.data(), lC.data(), lH.data(), n_nodes, C.data(), H.data(), root.com.data(),
                                           root.hash.data(), (int)p0.policy, (int)p0.aggregation_factor, p0.n_bits, R.data(), r_len, verify_seed, ok.data(),
                                           &unique));
        for (size_t e = 0; e < b; e++) out[e] = ok[e] != 0;
        return {out, unique};
    }
    std::optional<std::vector<DapolProof>> prove_many(const std::vector<uint64_t>& leaves, const Bytes32& nonce_seed, int n_bits, bool shared) const {
        size_t es = dapol_entity_proof_size(height_, (int)policy_, (int)aggregation_factor_, n_bits);
        if (es == 0) throw DapolError(DAPOL_ERR_INVALID_ARGUMENT);
        size_t b = leaves.size(), h = (size_t)height_;
        std::vector<uint8_t> C(b * h * 32), H(b * h * 32), R(b * es);
        int32_t rc = shared ? dapol_prove_entities_shared(ctx_->get(), tree_.get(), b, leaves.data(), (int)policy_, (int)aggregation_factor_, n_bits,
                                                          nonce_seed.data(), 0, nullptr, nullptr, nullptr, nullptr, C.data(), H.data(), R.data(), nullptr)
                            : dapol_prove_entities(ctx_->get(), tree_.get(), b, leaves.data(), (int)policy_, (int)aggregation_factor_, n_bits,
                                                   nonce_seed.data(), C.data(), H.data(), R.data());
        if (rc == DAPOL_ERR_UNKNOWN_LEAF) return std::nullopt;
        check(rc);
        return unpack(leaves, C, H, R, es, n_bits);
    }
    // [b][h][32] siblings + [b][es] blobs -> one DapolProof per leaf
    std::vector<DapolProof> unpack(const std::vector<uint64_t>& leaves, const std::vector<uint8_t>& C, const std::vector<uint8_t>& H, const std::vector<uint8_t>& R,
                                   size_t es, int n_bits) const {
        const size_t b = leaves.size(), h = (size_t)height_;
        std::vector<DapolProof> out(b);
        for (size_t e = 0; e < b; e++) {
            out[e].leaf_index = leaves[e];
            out[e].merkle_siblings.resize(h);
            for (size_t s = 0; s < h; s++) {
                std::memcpy(out[e].merkle_siblings[s].com.data(), &C[(e * h + s) * 32], 32);
                std::memcpy(out[e].merkle_siblings[s].hash.data(), &H[(e * h + s) * 32], 32);
            }
            out[e].range_proofs.assign(R.begin() + e * es, R.begin() + (e + 1) * es);
            out[e].policy = policy_; out[e].aggregation_factor = aggregation_factor_; out[e].n_bits = n_bits; out[e].height = height_;
        }
        return out;
    }
    // liabilities as the C ABI takes them: ids concatenated, with n + 1 offsets
    struct Packed {
        std::vector<uint8_t> iid, eid;
        std::vector<uint32_t> ioff, eoff;
        std::vector<uint64_t> vals;
        explicit Packed(const std::vector<Liability>& liabilities) : ioff(liabilities.size() + 1, 0), eoff(liabilities.size() + 1, 0), vals(liabilities.size()) {
            for (size_t i = 0; i < liabilities.size(); i++) {
                iid.insert(iid.end(), liabilities[i].internal_id.begin(), liabilities[i].internal_id.end());
                eid.insert(eid.end(), liabilities[i].external_id.begin(), liabilities[i].external_id.end());
                ioff[i + 1] = (uint32_t)iid.size();
                eoff[i + 1] = (uint32_t)eid.size();
                vals[i] = liabilities[i].value;
            }
            iid.push_back(0); eid.push_back(0);                             // never pass a null data pointer
        }
    };
    std::map<LiabilityId, uint64_t> id_to_idx_map_;
    int digest_ = DAPOL_DIGEST_BLAKE3;                   // create's digest and audit seed (created_: there are some)
    std::vector<uint8_t> audit_seed_;
    bool created_ = false;
    std::shared_ptr<Context> ctx_;
    std::shared_ptr<dapol_tree> tree_;
    int height_ = 0;
    size_t aggregation_factor_ = 0;
    Policy policy_ = Policy::Padding;
};

}  // namespace dapol
