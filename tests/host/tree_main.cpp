// The host side of the lineage tree (csrc/pa_tree.h) as a program of its own:
// validation, the preorder renumbering, the pairwise climb and the clade sums
// against brute force over root paths, on hand-made and random trees.  Built
// with AddressSanitizer and UBSan by tests/test_lineage_host.py; no GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pa_tree.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            return 1;                                                   \
        }                                                               \
    } while (0)

static std::vector<uint32_t> root_path(const std::vector<uint32_t> &parent, uint32_t v) {
    std::vector<uint32_t> p{v};
    while (v != 0) p.push_back(v = parent[v]);
    return std::vector<uint32_t>(p.rbegin(), p.rend());
}

static uint32_t brute_lca(const std::vector<uint32_t> &parent, uint32_t a, uint32_t b) {
    const std::vector<uint32_t> pa = root_path(parent, a), pb = root_path(parent, b);
    uint32_t v = 0;
    for (size_t i = 0; i < pa.size() && i < pb.size() && pa[i] == pb[i]; i++) v = pa[i];
    return v;
}

static int check_tree(const std::vector<uint32_t> &parent) {
    const uint32_t n = (uint32_t)parent.size();
    CHECK(pa::tree_check(parent.data(), n, nullptr, 0) == nullptr);
    const pa::Preorder t = pa::tree_preorder(parent.data(), n);
    std::vector<int> seen(n, 0);
    for (uint32_t v = 0; v < n; v++) {
        CHECK(t.pre[v] < n && !seen[t.pre[v]]++);
        CHECK(t.node_of[t.pre[v]] == v);
        CHECK(t.parent_pre[t.pre[v]] == t.pre[parent[v]]);
        CHECK(v == 0 || t.pre[parent[v]] < t.pre[v]);
    }
    CHECK(t.pre[0] == 0 && t.last[0] == n - 1);
    // the subtree of v is exactly the interval [pre[v], last[pre[v]]]; siblings ascend with their ids
    for (uint32_t v = 0; v < n; v++)
        for (uint32_t w = 0; w < n; w++) {
            const bool below = brute_lca(parent, v, w) == v;
            CHECK(below == (t.pre[v] <= t.pre[w] && t.pre[w] <= t.last[t.pre[v]]));
            if (v < w && v != 0 && parent[v] == parent[w]) CHECK(t.pre[v] < t.pre[w]);
        }
    for (uint32_t v = 0; v < n; v++)
        for (uint32_t w = 0; w < n; w++)
            CHECK(t.node_of[pa::tree_lca_pre(t, t.pre[v], t.pre[w])] == brute_lca(parent, v, w));
    std::vector<uint64_t> direct(n), clade(n), want(n, 0);
    for (uint32_t v = 0; v < n; v++) direct[v] = (uint64_t)v * 3 + 1;
    for (uint32_t v = 0; v < n; v++)
        for (uint32_t a : root_path(parent, v)) want[a] += direct[v];
    pa::tree_clade_sums(parent.data(), n, direct.data(), clade.data());
    CHECK(clade == want);
    return 0;
}

int main() {
    // what pa_lineage_create refuses
    const uint32_t one[] = {0}, bad_root[] = {1, 0}, self[] = {0, 1}, fwd[] = {0, 2, 0}, ok[] = {0, 0, 1};
    const uint32_t gn_ok[] = {2, 0, 2}, gn_bad[] = {0, 3};
    CHECK(pa::tree_check(one, 0, nullptr, 0) != nullptr);
    CHECK(pa::tree_check(one, 1, nullptr, 0) == nullptr);
    CHECK(pa::tree_check(bad_root, 2, nullptr, 0) != nullptr);
    CHECK(pa::tree_check(self, 2, nullptr, 0) != nullptr);
    CHECK(pa::tree_check(fwd, 3, nullptr, 0) != nullptr);
    CHECK(pa::tree_check(ok, 3, gn_ok, 3) == nullptr);
    CHECK(pa::tree_check(ok, 3, gn_bad, 2) != nullptr);
    // a hand-made tree: 0 -> {1, 2}, 1 -> {3, 5}, 2 -> {4}, 3 -> {6}: preorder 0 1 3 6 5 2 4
    const std::vector<uint32_t> hand{0, 0, 0, 1, 2, 1, 3};
    const pa::Preorder t = pa::tree_preorder(hand.data(), 7);
    const std::vector<uint32_t> order{0, 1, 3, 6, 5, 2, 4}, last{6, 4, 3, 3, 4, 6, 6};
    CHECK(t.node_of == order && t.last == last);
    if (check_tree(hand)) return 1;
    if (check_tree({0})) return 1;
    std::vector<uint32_t> chain(200), flat(200, 0);
    for (uint32_t i = 0; i < 200; i++) chain[i] = i ? i - 1 : 0;
    if (check_tree(chain) || check_tree(flat)) return 1;
    uint64_t s = 12345;
    for (int round = 0; round < 20; round++) {
        std::vector<uint32_t> parent(1 + (size_t)(round * 7) % 90, 0);
        for (uint32_t i = 1; i < parent.size(); i++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            parent[i] = (uint32_t)((s >> 33) % i);
        }
        if (check_tree(parent)) return 1;
    }
    std::printf("tree ok\n");
    return 0;
}
