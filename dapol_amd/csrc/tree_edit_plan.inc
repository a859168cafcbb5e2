// What the tree's edit paths (host_tree_edit.inc) decide on the host, as pure index arithmetic over what their first kernel reads
// back: which edits of a batch survive, the merged leaf set of a rebuild, the padding positions of a leaf set, and the plans of the
// in-place insert and remove.  No HIP call and no dapol_ctx: tests/cpp/tree_edit_plan_host.cpp prints these plans on the CPU and
// tests/test_tree_edit_plan_cpu.py checks them against a set model of the tree.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// The edits of a batch that survive, in leaf order: of several edits of one index the last wins.
static std::vector<uint32_t> sorted_last_wins(size_t k, const uint64_t* leaf_idx) {
    std::vector<uint32_t> ord(k), keep;
    for (size_t i = 0; i < k; i++) ord[i] = (uint32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return leaf_idx[a] < leaf_idx[b]; });
    for (size_t b = 0; b < k; b++)
        if (b + 1 == k || leaf_idx[ord[b + 1]] != leaf_idx[ord[b]]) keep.push_back(ord[b]);
    return keep;
}

struct HostLeaves {
    std::vector<uint64_t> idx, v;
    std::vector<uint8_t> r;              // [n][32]
    void push(uint64_t i, uint64_t value, const uint8_t* r32) { idx.push_back(i); v.push_back(value); r.insert(r.end(), r32, r32 + 32); }
};
// The sorted leaf set `old` with k edits applied, in input order: edit u puts (v[u], r32[u]) at leaf_idx[u] -- inserted, or replacing
// the leaf there (of several edits of one index the last wins).  v == nullptr: every edit REMOVES the leaf at its index instead
// (the caller has checked that each one is a leaf; a duplicate removes it once).
static void merge_leaf_edits(const HostLeaves& old, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32, HostLeaves& out) {
    const size_t n0 = old.idx.size();
    const std::vector<uint32_t> keep = sorted_last_wins(k, leaf_idx);
    out.idx.clear(); out.v.clear(); out.r.clear();
    out.idx.reserve(n0 + k); out.v.reserve(n0 + k); out.r.reserve((n0 + k) * 32);
    size_t a = 0, b = 0;
    while (a < n0 || b < keep.size()) {
        if (b < keep.size() && (a >= n0 || leaf_idx[keep[b]] <= old.idx[a])) {
            const uint32_t u = keep[b++];
            if (a < n0 && old.idx[a] == leaf_idx[u]) a++;         // replaces (or removes)
            if (v) out.push(leaf_idx[u], v[u], r32 + (size_t)u * 32);
        } else {
            out.push(old.idx[a], old.v[a], old.r.data() + a * 32);
            a++;
        }
    }
}

// Padding nodes of the tree over the given (sorted, distinct) leaves, in TAPE order: level bottom-up, index ascending (smtree's build
// restated: every real node's missing sibling is a padding node; a parent exists iff a child does).  level / index may be null.
static size_t padding_positions(int height, size_t n, const uint64_t* leaf_idx, uint8_t* level, uint64_t* index) {
    std::vector<uint64_t> cur(leaf_idx, leaf_idx + n), nxt;
    size_t k = 0;
    for (int L = 0; L < height; L++) {
        nxt.clear();
        for (size_t i = 0; i < cur.size();) {
            const uint64_t x = cur[i];
            if (!(x & 1) && i + 1 < cur.size() && cur[i + 1] == x + 1) i += 2;
            else {
                if (level) level[k] = (uint8_t)L;
                if (index) index[k] = x ^ 1ull;
                k++;
                i += 1;
            }
            nxt.push_back(x >> 1);
        }
        cur.swap(nxt);
    }
    return k;
}

// In-place insert of k new leaves (sorted, distinct, no two chains sharing a node), from what k_tree_ins_plan returns: m[j] = length of
// leaf j's chain of new nodes, inspos[j][t] = old-layout lower bound of chain node t < m[j], inspos[j][m[j]] = position of the first
// ancestor that exists.  Rows have H + 1 entries.
struct InsertPlan {
    int max_m = 0;
    std::vector<uint32_t> newpos;                // [k][H + 1]: t < m: chain node t in the NEW layout; [m]: the existing ancestor there
    std::vector<uint32_t> lvl_flat, lvl_off;     // levels 0 .. max_m: the insert positions (old layout) of the chains that reach the level, in
                                                 // leaf order; level t is lvl_flat[lvl_off[t] .. lvl_off[t + 1])
    uint32_t gained(int t) const { return lvl_off[t + 1] - lvl_off[t]; }
};
static InsertPlan plan_insert(size_t k, int H, const uint32_t* m, const uint32_t* inspos) {
    const size_t S1 = (size_t)H + 1;
    InsertPlan P;
    for (size_t j = 0; j < k; j++) P.max_m = std::max(P.max_m, (int)m[j]);
    std::vector<std::vector<uint32_t>> lvl((size_t)P.max_m + 1);
    P.newpos.assign(k * S1, 0);
    for (size_t j = 0; j < k; j++)
        for (int t = 0; t < (int)m[j]; t++) {
            P.newpos[j * S1 + t] = inspos[j * S1 + t] + (uint32_t)lvl[t].size();
            lvl[t].push_back(inspos[j * S1 + t]);
        }
    for (size_t j = 0; j < k; j++) {                         // the existing ancestor at level m_j, moved by what its level gains
        const int mj = (int)m[j];
        const uint32_t p = inspos[j * S1 + mj];
        P.newpos[j * S1 + mj] = p + (uint32_t)(std::upper_bound(lvl[mj].begin(), lvl[mj].end(), p) - lvl[mj].begin());
    }
    for (auto& l : lvl) { P.lvl_off.push_back((uint32_t)P.lvl_flat.size()); P.lvl_flat.insert(P.lvl_flat.end(), l.begin(), l.end()); }
    P.lvl_off.push_back((uint32_t)P.lvl_flat.size());
    return P;
}

// In-place removal of k leaves (si sorted, distinct), from what k_tree_rm_find returns: pos[j][t] / has_pad[j][t] = position and
// has_pad flag of leaf j's ancestor at level t, old layout; rows have H + 1 entries.  The touched nodes of level t are the distinct
// pos[j][t] in order (the leaves are sorted, so are their ancestors' positions).  A node dies iff all its real children die; a dead
// node whose parent survives is a chain top, and its surviving sibling S takes a padding node.
struct RemovePlan {
    bool ok = false;                             // false: the root died (an internal error; nothing else of the plan is set)
    int D = 0;                                   // levels 0 .. D - 1 lose nodes
    std::vector<std::vector<uint32_t>> dead;     // [H + 1]: the positions that go, old layout, ascending
    std::vector<std::vector<uint32_t>> merge;    // [H + 1]: (survivor at t, one of its surviving children at t - 1) pairs, new layout
    std::vector<uint32_t> pad_pos;               // chain tops: the surviving sibling S at level pad_lvl, new layout
    std::vector<uint8_t> pad_lvl;
    // one upload: 8 words for the pad seed | dead lists | pad positions | merge pairs
    std::vector<uint32_t> flat;
    std::vector<size_t> dead_off, merge_off;     // [H + 2]: list t is flat[off[t] .. off[t + 1])
    size_t pad_off = 0;
};
static RemovePlan plan_remove(int H, size_t k, const uint64_t* si, const uint32_t* pos, const uint8_t* has_pad) {
    const size_t S1 = (size_t)H + 1;
    RemovePlan P;
    P.dead.resize(S1); P.merge.resize(S1);
    struct Node { uint32_t pos, rep; bool dead; };             // rep = the first removed leaf under the node
    std::vector<Node> cur, nxt;
    for (size_t j = 0; j < k; j++) { cur.push_back({pos[j * S1], (uint32_t)j, true}); P.dead[0].push_back(pos[j * S1]); }
    for (int t = 0; t < H; t++) {
        nxt.clear();
        for (size_t a = 0; a < cur.size();) {                  // a parent has one or two touched children
            const uint32_t par = pos[cur[a].rep * S1 + t + 1];
            size_t b = a + 1;
            while (b < cur.size() && pos[cur[b].rep * S1 + t + 1] == par) b++;
            const Node c0 = cur[a];
            bool pdead, top = false;
            uint32_t child = 0;                                // a surviving child of a surviving parent
            if (b - a == 2) {                                  // both children touched
                const Node c1 = cur[a + 1];
                pdead = c0.dead && c1.dead;
                child = c0.dead ? c1.pos : c0.pos;
                top = c0.dead != c1.dead;
            } else {
                pdead = c0.dead && has_pad[c0.rep * S1 + t];   // a node with has_pad has one real child
                top = c0.dead && !pdead;
                child = !top ? c0.pos : ((si[c0.rep] >> t) & 1) ? c0.pos - 1 : c0.pos + 1;     // S: the real neighbour
            }
            if (top) { P.pad_lvl.push_back((uint8_t)t); P.pad_pos.push_back(child); }
            if (pdead) P.dead[t + 1].push_back(par);
            else { P.merge[t + 1].push_back(par); P.merge[t + 1].push_back(child); }
            nxt.push_back({par, c0.rep, pdead});
            a = b;
        }
        std::swap(cur, nxt);
    }
    if (!P.dead[H].empty()) return P;
    P.ok = true;
    while (P.D < H && !P.dead[P.D].empty()) P.D++;
    // old -> new positions: minus the deletions before
    auto newpos = [&](int t, uint32_t o) { return o - (uint32_t)(std::lower_bound(P.dead[t].begin(), P.dead[t].end(), o) - P.dead[t].begin()); };
    for (size_t i = 0; i < P.pad_pos.size(); i++) P.pad_pos[i] = newpos(P.pad_lvl[i], P.pad_pos[i]);
    for (int t = 1; t <= H; t++)
        for (size_t i = 0; i < P.merge[t].size(); i += 2) { P.merge[t][i] = newpos(t, P.merge[t][i]); P.merge[t][i + 1] = newpos(t - 1, P.merge[t][i + 1]); }
    P.flat.assign(8, 0);
    for (auto& d : P.dead) { P.dead_off.push_back(P.flat.size()); P.flat.insert(P.flat.end(), d.begin(), d.end()); }
    P.dead_off.push_back(P.flat.size());
    P.pad_off = P.flat.size();
    P.flat.insert(P.flat.end(), P.pad_pos.begin(), P.pad_pos.end());
    for (auto& g : P.merge) { P.merge_off.push_back(P.flat.size()); P.flat.insert(P.flat.end(), g.begin(), g.end()); }
    P.merge_off.push_back(P.flat.size());
    return P;
}
