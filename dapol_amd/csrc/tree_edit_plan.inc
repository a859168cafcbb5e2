// What the tree's edit paths (host_tree_edit.inc) decide on the host, as pure index arithmetic over what their first kernel reads
// back: which edits of a batch survive, the merged leaf set of a rebuild, the padding positions of a leaf set, and the plans of the
// in-place insert, remove and mixed edit.  No HIP call and no dapol_ctx: tests/cpp/tree_edit_plan_host.cpp (tree_insert_plan_host.cpp,
// tree_apply_plan_host.cpp) prints these plans on the CPU and tests/test_tree_edit_plan_cpu.py (test_tree_insert_plan_cpu.py,
// test_tree_apply_plan_cpu.py) checks them against a set model of the tree.
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
// (the caller has checked that each one is a leaf; a duplicate removes it once).  drop (may be null; a mixed edit, dapol_tree_apply): edit
// u with drop[u] != 0 removes the leaf at its index, the others put theirs.
static void merge_leaf_edits(const HostLeaves& old, size_t k, const uint64_t* leaf_idx, const uint64_t* v, const uint8_t* r32, HostLeaves& out,
                             const uint8_t* drop = nullptr) {
    const size_t n0 = old.idx.size();
    const std::vector<uint32_t> keep = sorted_last_wins(k, leaf_idx);
    out.idx.clear(); out.v.clear(); out.r.clear();
    out.idx.reserve(n0 + k); out.v.reserve(n0 + k); out.r.reserve((n0 + k) * 32);
    size_t a = 0, b = 0;
    while (a < n0 || b < keep.size()) {
        if (b < keep.size() && (a >= n0 || leaf_idx[keep[b]] <= old.idx[a])) {
            const uint32_t u = keep[b++];
            if (a < n0 && old.idx[a] == leaf_idx[u]) a++;         // replaces (or removes)
            if (v && !(drop && drop[u])) out.push(leaf_idx[u], v[u], r32 + (size_t)u * 32);
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

// In-place insert of k new leaves (sorted, distinct, no two chains sharing a node), from what k_tree_ins_plan<true> returns: m[j] = length of
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

// In-place removal of k leaves (si sorted, distinct), from what k_tree_find_paths returns: pos[j][t] / has_pad[j][t] = position and
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

// In-place insert of k new leaves in general -- chains may share nodes (a sibling pair, a whole new subtree) -- from what
// k_tree_ins_plan<false> returns: x = the indexes, sorted and distinct; m[j] = length of leaf j's chain of new nodes; pos_all[j][t] = the
// old-layout lower bound of x[j] >> t at every level t <= H (for t >= m[j] the ancestor's exact position).  Rows have H + 1 entries.
//   The FRESH nodes of level t are the distinct x[j] >> t in ascending order: the new ones (t < m[j]) and, above them, the existing
// ancestors the call has to merge again.  A fresh node's position in the new layout is its lower bound plus the number of NEW nodes
// before it in that list (for an existing node these are exactly the new nodes with a smaller index).  A new node has a padding
// sibling iff its parent is new and its sibling is not; a new node whose parent exists is a TOP: its sibling S is an existing real
// node, adjacent in the sorted level, which carries the padding record of the top's position and loses has_pad.  Every fresh node
// above the leaves is merged from its children; a fresh node's slot (where its extended point waits for the merge above) is its rank
// in its level's fresh list, a padding node's slot its rank in the pad list.
struct InsertGeneralPlan {
    enum : uint32_t { NONE = 0xffffffffu, PAD_SLOT = 0x80000000u };
    int D = 0;                                   // levels 0 .. D - 1 gain nodes
    uint32_t max_fresh = 0;                      // the longest fresh list (slots per level)
    std::vector<std::vector<uint32_t>> gain;     // [H + 1]: old-layout lower bounds of the level's new nodes, ascending
    // per new node, level by level bottom-up, index ascending
    std::vector<uint32_t> n_lvl, n_pos, n_parent, n_sib;     // level | new position | parent's new position | tops: S's new position, else NONE
    std::vector<uint64_t> n_idx;
    std::vector<uint8_t> n_has_pad;
    std::vector<uint32_t> leaf_pos;              // [k]: new position of leaf j (its slot is j)
    std::vector<uint32_t> pad_lvl, pad_pos;      // the new nodes that take a padding sibling, in the order above; pad slot = rank here
    // [H + 1], level t >= 1: five words per fresh node of the level --
    //   its new position | new position of its first fresh child (level t - 1) | its slot | that child's slot |
    //   the other child: a slot of level t - 1 (fresh too), PAD_SLOT | pad slot (the child's new padding sibling), or NONE (an
    //   untouched node or an old padding record: decoded from the level's arrays)
    std::vector<std::vector<uint32_t>> merge;
    // one upload: 8 words for the pad seed | gain lists | n_lvl | n_pos | n_parent | n_sib | n_idx lo | n_idx hi | leaf_pos | pad_lvl | pad_pos | merge lists
    std::vector<uint32_t> flat;
    std::vector<size_t> gain_off, merge_off;     // [H + 2]: list t is flat[off[t] .. off[t + 1])
    size_t lvl_off = 0, pos_off = 0, parent_off = 0, sib_off = 0, idx_lo_off = 0, idx_hi_off = 0, leaf_off = 0, pad_lvl_off = 0, pad_pos_off = 0;
};
static InsertGeneralPlan plan_insert_general(int H, size_t k, const uint64_t* x, const uint32_t* m, const uint32_t* pos_all) {
    const size_t S1 = (size_t)H + 1;
    InsertGeneralPlan P;
    P.gain.resize(S1); P.merge.resize(S1);
    auto shr = [](uint64_t a, int t) { return t < 64 ? a >> t : (uint64_t)0; };
    struct Fresh { uint32_t rep, pos; bool is_new; uint32_t node; };     // rep = the first new leaf under it; node = its row in n_* (new nodes)
    std::vector<Fresh> cur, nxt;
    auto fresh_of = [&](int t, std::vector<Fresh>& out) {
        out.clear();
        uint32_t n_new = 0;
        for (size_t j = 0; j < k; j++) {
            if (j > 0 && shr(x[j], t) == shr(x[j - 1], t)) continue;
            const bool is_new = t < (int)m[j];
            const uint32_t lb = pos_all[j * S1 + t];
            out.push_back({(uint32_t)j, lb + n_new, is_new, InsertGeneralPlan::NONE});
            if (is_new) { P.gain[t].push_back(lb); n_new++; }
        }
    };
    fresh_of(0, cur);
    for (int t = 0; t <= H; t++) {
        if (t < H) fresh_of(t + 1, nxt); else nxt.clear();
        P.max_fresh = std::max(P.max_fresh, (uint32_t)cur.size());
        // parents: fresh node a of level t hangs under nxt[q], q advancing with the parent's index
        size_t q = 0;
        for (size_t a = 0; a < cur.size(); a++) {
            Fresh& c = cur[a];
            const uint64_t me = shr(x[c.rep], t);
            if (t < H) while (shr(x[nxt[q].rep], t + 1) != me >> 1) q++;
            if (t == 0) P.leaf_pos.push_back(c.pos);
            if (!c.is_new) continue;
            const bool sib_new = (a > 0 && cur[a - 1].is_new && shr(x[cur[a - 1].rep], t) == (me ^ 1)) ||
                                 (a + 1 < cur.size() && cur[a + 1].is_new && shr(x[cur[a + 1].rep], t) == (me ^ 1));
            const bool parent_new = nxt[q].is_new;            // (a new node is never the root: t < m <= H)
            const bool has_pad = parent_new && !sib_new;
            c.node = (uint32_t)P.n_pos.size();
            P.n_lvl.push_back((uint32_t)t); P.n_pos.push_back(c.pos); P.n_idx.push_back(me); P.n_parent.push_back(nxt[q].pos);
            P.n_sib.push_back(parent_new ? InsertGeneralPlan::NONE : (me & 1) ? c.pos - 1 : c.pos + 1);
            P.n_has_pad.push_back(has_pad);
            if (has_pad) { P.pad_lvl.push_back((uint32_t)t); P.pad_pos.push_back(c.pos); }
        }
        if (t == H) break;
        // merges of level t + 1: the one or two fresh children of every fresh node there
        uint32_t pad_slot = (uint32_t)P.pad_pos.size();
        for (size_t a = cur.size(); a-- > 0;) if (cur[a].is_new && P.n_has_pad[cur[a].node]) cur[a].node = --pad_slot; else cur[a].node = InsertGeneralPlan::NONE;   // node := pad slot
        for (size_t a = 0, qq = 0; a < cur.size(); qq++) {
            const uint64_t par = shr(x[cur[a].rep], t) >> 1;
            const bool two = a + 1 < cur.size() && (shr(x[cur[a + 1].rep], t) >> 1) == par;
            const uint32_t other = two ? (uint32_t)(a + 1) : cur[a].node != InsertGeneralPlan::NONE ? (InsertGeneralPlan::PAD_SLOT | cur[a].node) : InsertGeneralPlan::NONE;
            const uint32_t e[5] = {nxt[qq].pos, cur[a].pos, (uint32_t)qq, (uint32_t)a, other};
            P.merge[t + 1].insert(P.merge[t + 1].end(), e, e + 5);
            a += two ? 2 : 1;
        }
        std::swap(cur, nxt);
    }
    while (P.D < H && !P.gain[P.D].empty()) P.D++;
    P.flat.assign(8, 0);
    auto put = [&](const std::vector<uint32_t>& v) { const size_t o = P.flat.size(); P.flat.insert(P.flat.end(), v.begin(), v.end()); return o; };
    for (auto& g : P.gain) P.gain_off.push_back(put(g));
    P.gain_off.push_back(P.flat.size());
    P.lvl_off = put(P.n_lvl); P.pos_off = put(P.n_pos); P.parent_off = put(P.n_parent); P.sib_off = put(P.n_sib);
    P.idx_lo_off = P.flat.size();
    for (uint64_t i : P.n_idx) P.flat.push_back((uint32_t)i);
    P.idx_hi_off = P.flat.size();
    for (uint64_t i : P.n_idx) P.flat.push_back((uint32_t)(i >> 32));
    P.leaf_off = put(P.leaf_pos); P.pad_lvl_off = put(P.pad_lvl); P.pad_pos_off = put(P.pad_pos);
    for (auto& g : P.merge) P.merge_off.push_back(put(g));
    P.merge_off.push_back(P.flat.size());
    return P;
}

// In-place MIXED edit (dapol_tree_apply): removals, new leaves and replacements as one plan, from what k_tree_apply_plan returns for
// the sorted, distinct union x of the edited indexes: is_put[j] (1 = a put, 0 = a removal, whose leaf exists -- the caller has checked),
// lb[j][t] = old-layout lower bound of x[j] >> t at every level t <= H, fl[j][t] bit 0 = that node exists, bit 1 = its has_pad flag.
// Rows have H + 1 entries.
//   The TOUCHED nodes of level t are the distinct x[j] >> t, ascending.  A touched node is ALIVE afterwards iff a leaf of the new set
// lies under it: a put at level 0; above, a touched child that is alive or an untouched real child (an old node's real children are
// counted by has_pad, as in plan_remove).  So a touched node is one of: a survivor (exists, alive -- also when every old leaf under it
// goes and a put lands there), dead (exists, not alive) or born (did not exist, alive).  New position of a survivor or born node = its
// lower bound + born nodes before it - dead nodes before it.  has_pad of every alive touched node is "the sibling is absent
// afterwards"; an UNTOUCHED real sibling S of a touched node changes with it: S gains a padding sibling beside a node that dies and
// loses it beside one that is born.  A padding node is made wherever has_pad holds afterwards and the old tree did not hold the
// record of that very position (an old node with has_pad set: the record is still right and moves with its node).
//   Every alive touched node above the leaves is merged from an ANCHOR child -- its first alive touched child, else the untouched S
// beside a dead one -- and the anchor's other child; a child this call has made (touched node, put leaf, new padding node) waits in a
// slot: a touched node's slot is its rank among its level's alive touched nodes, a padding node's its rank in the pad list.
struct ApplyPlan {
    enum : uint32_t { NONE = 0xffffffffu, PAD_SLOT = 0x80000000u };
    bool ok = false;                             // false: the root died (the caller refuses a batch that leaves no leaf before planning)
    int D = 0;                                   // levels 0 .. D - 1 are rewritten: D - 1 is the highest level that gains or loses a node
    uint32_t max_slots = 0;                      // the most alive touched nodes of one level
    std::vector<std::vector<uint32_t>> dead;     // [H + 1]: old positions of the nodes that go, ascending
    std::vector<std::vector<uint32_t>> born;     // [H + 1]: old-layout lower bounds of the nodes that come, ascending
    // structure records, level by level bottom-up, position ascending: every alive touched node below the root, and every S whose
    // has_pad changes.  s_flag bit 0: born (idx and parent are written), bit 1: has_pad afterwards.  s_parent: NONE unless born.
    std::vector<uint32_t> s_lvl, s_pos, s_parent, s_flag;
    std::vector<uint64_t> s_idx;
    std::vector<uint32_t> put_pos;               // per put, in index order: its leaf's new position (its slot is its rank among the puts)
    std::vector<uint8_t> put_new;                // ... and whether the leaf is new
    std::vector<uint32_t> pad_lvl, pad_pos;      // the real nodes (new positions) that take a new padding sibling, in the order above
    // [H + 1], level t >= 1: five words per alive touched node of the level --
    //   its new position | new position of the anchor child (level t - 1) | its slot | the anchor's slot, or NONE (S: decoded) |
    //   the other child: a slot of level t - 1, PAD_SLOT | pad slot, or NONE (an untouched real node or an old padding record: decoded)
    std::vector<std::vector<uint32_t>> merge;
    // one upload: 8 words for the pad seed | dead lists | born lists | s_lvl | s_pos | s_parent | s_flag | s_idx lo | s_idx hi | put_pos | pad_lvl | pad_pos | merge lists
    std::vector<uint32_t> flat;
    std::vector<size_t> dead_off, born_off, merge_off;     // [H + 2]: list t is flat[off[t] .. off[t + 1])
    size_t lvl_off = 0, pos_off = 0, parent_off = 0, flag_off = 0, idx_lo_off = 0, idx_hi_off = 0, put_off = 0, pad_lvl_off = 0, pad_pos_off = 0;
};
static ApplyPlan plan_apply(int H, size_t k, const uint64_t* x, const uint8_t* is_put, const uint32_t* lb, const uint8_t* fl) {
    const size_t S1 = (size_t)H + 1;
    ApplyPlan P;
    P.dead.resize(S1); P.born.resize(S1); P.merge.resize(S1);
    auto shr = [](uint64_t a, int t) { return t < 64 ? a >> t : (uint64_t)0; };
    struct Node {
        uint32_t rep;                            // the first edited index under the node
        uint64_t idx;
        bool exists, hp_old, alive;
        uint32_t pos = 0, slot = ApplyPlan::NONE;                  // new position and slot (alive nodes)
        bool has_pad = false;                    // afterwards
        uint32_t pad_slot = ApplyPlan::NONE;     // the padding sibling this call makes for it
        bool s_real = false;                     // its sibling is an untouched real node S ...
        uint32_t s_pos = 0, s_pad_slot = ApplyPlan::NONE;          // ... at this new position, which takes this new padding node
    };
    std::vector<Node> cur, nxt;
    auto touched = [&](int t, std::vector<Node>& out) {           // the level's touched nodes; `alive` is the caller's to set
        out.clear();
        for (size_t j = 0; j < k; j++) {
            if (j > 0 && shr(x[j], t) == shr(x[j - 1], t)) continue;
            Node n;
            n.rep = (uint32_t)j; n.idx = shr(x[j], t);
            n.exists = fl[j * S1 + t] & 1; n.hp_old = n.exists && (fl[j * S1 + t] & 2); n.alive = false;
            out.push_back(n);
        }
    };
    auto place = [&](int t, std::vector<Node>& lv) {              // new positions and slots, the level's dead and born lists
        uint32_t n_born = 0, n_dead = 0, n_alive = 0;
        for (Node& n : lv) {
            const uint32_t l = lb[n.rep * S1 + t];
            n.pos = l + n_born - n_dead;
            if (n.alive) n.slot = n_alive++;
            if (n.alive && !n.exists) { P.born[t].push_back(l); n_born++; }
            if (!n.alive && n.exists) { P.dead[t].push_back(l); n_dead++; }
        }
        P.max_slots = std::max(P.max_slots, n_alive);
    };
    touched(0, cur);
    for (Node& n : cur) n.alive = is_put[n.rep] != 0;
    for (Node& n : cur) if (n.alive) P.put_new.push_back(!n.exists);
    place(0, cur);
    for (const Node& n : cur) if (n.alive) P.put_pos.push_back(n.pos);
    for (int t = 0; t < H; t++) {
        // siblings: who is beside every touched node afterwards
        uint32_t n_born = 0, n_dead = 0;
        for (size_t a = 0; a < cur.size(); a++) {
            Node& n = cur[a];
            const bool born = n.alive && !n.exists, dead = !n.alive && n.exists;
            const Node* sib = a > 0 && cur[a - 1].idx == (n.idx ^ 1) ? &cur[a - 1] : a + 1 < cur.size() && cur[a + 1].idx == (n.idx ^ 1) ? &cur[a + 1] : nullptr;
            bool sib_after;
            if (sib) sib_after = sib->alive;
            else {
                // untouched: it exists iff the old node has no padding sibling, or -- beside a node that did not exist -- iff the parent did
                n.s_real = sib_after = n.exists ? !n.hp_old : (fl[n.rep * S1 + t + 1] & 1) != 0;
                if (n.s_real) {
                    const uint32_t l = lb[n.rep * S1 + t];
                    const bool s_right = (n.idx & 1) == 0;
                    const uint32_t s_old = s_right ? l + (n.exists ? 1 : 0) : l - 1;
                    n.s_pos = s_right ? s_old + n_born + (born ? 1 : 0) - n_dead - (dead ? 1 : 0) : s_old + n_born - n_dead;
                }
            }
            n.has_pad = n.alive && !sib_after;
            n_born += born; n_dead += dead;
        }
        // the level above: alive iff a child is
        touched(t + 1, nxt);
        {
            size_t q = 0;
            for (const Node& n : cur) {
                while (nxt[q].idx != n.idx >> 1) q++;
                if (n.alive || n.s_real) nxt[q].alive = true;
            }
        }
        place(t + 1, nxt);
        // structure records and padding nodes of level t
        {
            size_t q = 0;
            for (Node& n : cur) {
                while (nxt[q].idx != n.idx >> 1) q++;
                const bool born = n.alive && !n.exists, dead = !n.alive && n.exists;
                const bool s_changes = n.s_real && (born || dead);
                auto s_record = [&] {
                    P.s_lvl.push_back((uint32_t)t); P.s_pos.push_back(n.s_pos); P.s_parent.push_back(ApplyPlan::NONE); P.s_flag.push_back(dead ? 2u : 0u);
                    P.s_idx.push_back(n.idx ^ 1);
                    if (dead) { n.s_pad_slot = (uint32_t)P.pad_pos.size(); P.pad_lvl.push_back((uint32_t)t); P.pad_pos.push_back(n.s_pos); }
                };
                if (s_changes && (n.idx & 1)) s_record();         // S on the left comes first
                if (n.alive) {
                    P.s_lvl.push_back((uint32_t)t); P.s_pos.push_back(n.pos); P.s_parent.push_back(born ? nxt[q].pos : ApplyPlan::NONE);
                    P.s_flag.push_back((born ? 1u : 0u) | (n.has_pad ? 2u : 0u));
                    P.s_idx.push_back(n.idx);
                    if (n.has_pad && !n.hp_old) { n.pad_slot = (uint32_t)P.pad_pos.size(); P.pad_lvl.push_back((uint32_t)t); P.pad_pos.push_back(n.pos); }
                }
                if (s_changes && !(n.idx & 1)) s_record();
            }
        }
        // merges of level t + 1
        for (size_t a = 0, q = 0; a < cur.size(); q++) {
            size_t b = a + 1;
            if (b < cur.size() && (cur[b].idx >> 1) == (cur[a].idx >> 1)) b++;
            const Node& par = nxt[q];
            if (par.alive) {
                const Node* an = cur[a].alive ? &cur[a] : b - a == 2 && cur[a + 1].alive ? &cur[a + 1] : nullptr;
                uint32_t e[5] = {par.pos, 0, par.slot, ApplyPlan::NONE, ApplyPlan::NONE};
                if (an) {
                    const Node* sib = b - a == 2 ? (an == &cur[a] ? &cur[a + 1] : &cur[a]) : nullptr;
                    e[1] = an->pos; e[3] = an->slot;
                    if (an->has_pad) e[4] = an->pad_slot != ApplyPlan::NONE ? (ApplyPlan::PAD_SLOT | an->pad_slot) : ApplyPlan::NONE;
                    else if (sib) e[4] = sib->slot;
                } else {                                          // S beside a dead node: decoded, with the padding node just made for it
                    e[1] = cur[a].s_pos;
                    e[4] = ApplyPlan::PAD_SLOT | cur[a].s_pad_slot;
                }
                P.merge[t + 1].insert(P.merge[t + 1].end(), e, e + 5);
            }
            a = b;
        }
        std::swap(cur, nxt);
    }
    if (cur.size() != 1 || !cur[0].alive) return P;              // (H == 0: the one leaf was removed)
    P.ok = true;
    for (int t = 0; t <= H; t++) if (!P.dead[t].empty() || !P.born[t].empty()) P.D = t + 1;
    P.flat.assign(8, 0);
    auto put = [&](const std::vector<uint32_t>& v) { const size_t o = P.flat.size(); P.flat.insert(P.flat.end(), v.begin(), v.end()); return o; };
    for (auto& g : P.dead) P.dead_off.push_back(put(g));
    P.dead_off.push_back(P.flat.size());
    for (auto& g : P.born) P.born_off.push_back(put(g));
    P.born_off.push_back(P.flat.size());
    P.lvl_off = put(P.s_lvl); P.pos_off = put(P.s_pos); P.parent_off = put(P.s_parent); P.flag_off = put(P.s_flag);
    P.idx_lo_off = P.flat.size();
    for (uint64_t i : P.s_idx) P.flat.push_back((uint32_t)i);
    P.idx_hi_off = P.flat.size();
    for (uint64_t i : P.s_idx) P.flat.push_back((uint32_t)(i >> 32));
    P.put_off = put(P.put_pos); P.pad_lvl_off = put(P.pad_lvl); P.pad_pos_off = put(P.pad_pos);
    for (auto& g : P.merge) P.merge_off.push_back(put(g));
    P.merge_off.push_back(P.flat.size());
    return P;
}
