// pa_tree_dev.h -- the device side of the lineage tree:
// the preorder tables of a pa_lineage and the climb that turns the smallest and
// the largest preorder number of a node set into its lowest common ancestor.
// Shared by the reads' reduction (pa_lineage.hip) and the k-mers' (pa_contain.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pad {

struct TreeDev {
    const uint32_t *parent, *last, *node_of, *gpre;  // [n_nodes] x 3 by preorder number; [G]
    uint32_t n_nodes, G;
};

// The climb from the smaller preorder number until the subtree's interval holds
// the larger; the caller's node.  mn <= mx < n_nodes; the root's interval holds
// every number, so the loop ends there at the latest.
__device__ __forceinline__ uint32_t climb(const TreeDev &t, uint32_t mn, uint32_t mx) {
    uint32_t v = mn;
    while (t.last[v] < mx && v != 0) v = t.parent[v];
    return t.node_of[v];
}

}  // namespace pad
