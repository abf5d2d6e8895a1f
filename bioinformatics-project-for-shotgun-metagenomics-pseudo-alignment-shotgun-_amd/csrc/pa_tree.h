// pa_tree.h -- the host side of the lineage tree: its
// validation, the depth-first preorder renumbering and the clade sums.  Plain
// C++ with no HIP in it, so it also builds into a stand-alone host program
// (tests/host/tree_main.cpp).
#pragma once

#include <stdint.h>

#include <vector>

namespace pa {

// nullptr for a tree pa_lineage_create accepts, else what is wrong with it:
// nodes 0 .. n_nodes - 1, node 0 the root (its own parent), parent[i] < i for
// i >= 1, every genome on a node of the tree.
inline const char *tree_check(const uint32_t *parent, uint64_t n_nodes, const uint32_t *genome_node,
                              uint64_t n_genomes) {
    if (n_nodes == 0) return "a tree has at least one node (n_nodes == 0)";
    if (parent[0] != 0) return "node 0 is the root: parent[0] must be 0";
    for (uint64_t i = 1; i < n_nodes; i++)
        if (parent[i] >= i) return "parent[i] must be smaller than i for every node i >= 1";
    for (uint64_t g = 0; g < n_genomes; g++)
        if (genome_node[g] >= n_nodes) return "genome_node[g] must be a node of the tree";
    return nullptr;
}

// The nodes of a checked tree in depth-first preorder, children in ascending
// node number.  pre[v]: v's preorder number; node_of[t]: the node numbered t;
// parent_pre[t] / last[t]: the preorder number of that node's parent (the
// root: 0) and the largest preorder number in its subtree, so that the subtree
// of the node numbered t is exactly the interval [t, last[t]].
struct Preorder {
    std::vector<uint32_t> pre, node_of, parent_pre, last;
};
inline Preorder tree_preorder(const uint32_t *parent, uint32_t n) {
    Preorder o;
    std::vector<uint32_t> size(n, 1), next(n, 0);
    for (uint32_t i = n; i-- > 1;) size[parent[i]] += size[i];  // (parent[i] < i: every child before its parent)
    o.pre.assign(n, 0), o.node_of.assign(n, 0), o.parent_pre.assign(n, 0), o.last.assign(n, 0);
    next[0] = 1;
    for (uint32_t i = 1; i < n; i++) {  // (ascending: a node after its parent, siblings in node order)
        const uint32_t p = parent[i];
        o.pre[i] = next[p];
        next[p] += size[i];
        next[i] = o.pre[i] + 1;
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t t = o.pre[i];
        o.node_of[t] = i;
        o.parent_pre[t] = o.pre[parent[i]];
        o.last[t] = t + size[i] - 1;
    }
    return o;
}

// clade[v] = the sum of direct over v's subtree, bottom-up over parent[i] < i.
inline void tree_clade_sums(const uint32_t *parent, uint32_t n, const uint64_t *direct, uint64_t *clade) {
    for (uint32_t i = 0; i < n; i++) clade[i] = direct[i];
    for (uint32_t i = n; i-- > 1;) clade[parent[i]] += clade[i];
}

// The lowest common ancestor of the nodes numbered a and b (preorder numbers):
// a climb from the smaller until its subtree's interval holds the larger.
inline uint32_t tree_lca_pre(const Preorder &t, uint32_t a, uint32_t b) {
    uint32_t v = a < b ? a : b;
    const uint32_t hi = a < b ? b : a;
    while (t.last[v] < hi) v = t.parent_pre[v];
    return v;
}

}  // namespace pa
