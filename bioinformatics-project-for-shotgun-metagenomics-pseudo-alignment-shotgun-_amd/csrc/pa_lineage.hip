// pa_lineage.hip -- lineages: every read's node in a taxonomy tree and the
// reads counted per node.  DESIGN.md section 17.
//
//   tree       the caller's nodes renumbered in depth-first preorder once, at
//              creation (pa_tree.h): a subtree is then an interval [t, last[t]]
//              of preorder numbers, and the lowest common ancestor of any node
//              set is that of its smallest and its largest number.
//   sets       candidates_device (pa_abund.hip) leaves every read's type and
//              compatibility set C(r) on the device: one genome for a unique
//              read, section 14's set for an ambiguous one, none otherwise.
//   reduction  k_lineage_lane, a lane per read: the min and max preorder number
//              over a short set, the climb, the node.  A set longer than
//              kLaneSet is queued (one atomic per wave) for k_lineage_wave, a
//              wave per read: the lanes scan the set coalesced, a wave min / max.
//   counts     direct[node] += 1 per classified read: a uint32 histogram in LDS
//              flushed once per workgroup for trees of up to
//              PA_LINEAGE_LDS_NODES nodes, 64-bit global atomics above.  Integer
//              atomics only: the counts do not depend on the batches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <new>

#include "pa_device.h"
#include "pa_internal.h"
#include "pa_tree.h"
#include "pa_tree_dev.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNoNode = PA_NO_NODE;
// A lane scans a set of up to this many genomes itself; longer ones go to a wave.
// At 16 a lane's scan is one 64-byte line of the sets; a wave's coalesced scan
// covers the same 16 genomes in a quarter of one load instruction.
constexpr uint32_t kLaneSet = 16;

using pad::climb;  // (pa_tree_dev.h: the k-mers' reduction of pa_contain.hip climbs the same tables)
using pad::TreeDev;

template <bool LDS>
__device__ __forceinline__ void count_node(uint32_t *hist, unsigned long long *direct, uint32_t node) {
    if (LDS)
        atomicAdd(&hist[node], 1u);
    else
        atomicAdd(&direct[node], 1ull);
}

template <bool LDS>
__device__ __forceinline__ void hist_clear(uint32_t *hist, uint32_t n_nodes) {
    if (LDS) {
        for (uint32_t v = threadIdx.x; v < n_nodes; v += kBlock) hist[v] = 0;
        __syncthreads();
    }
}

template <bool LDS>
__device__ __forceinline__ void hist_flush(const uint32_t *hist, unsigned long long *direct, uint32_t n_nodes) {
    if (LDS) {
        __syncthreads();
        for (uint32_t v = threadIdx.x; v < n_nodes; v += kBlock)
            if (hist[v]) atomicAdd(&direct[v], (unsigned long long)hist[v]);
    }
}

// A lane per set.  type: the reads' mapping types, or null (pa_lineage_lca: sets
// alone).  queue / qcount: the sets left to k_lineage_wave.  err bit 0: a genome
// outside the index; bit 1: an ambiguous read with an empty set.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_lineage_lane(const uint8_t *__restrict__ type,
                                                         const uint64_t *__restrict__ set_off,
                                                         const uint32_t *__restrict__ sets, uint64_t n, uint64_t total,
                                                         TreeDev t, uint32_t *__restrict__ node_out,
                                                         unsigned long long *__restrict__ direct,
                                                         uint32_t *__restrict__ queue, unsigned long long *qcount,
                                                         uint32_t *err) {
    extern __shared__ uint32_t lineage_hist[];
    hist_clear<LDS>(lineage_hist, t.n_nodes);
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = base + threadIdx.x;
        uint64_t o = 0, e = 0;
        if (i < n) {
            o = set_off[i], e = set_off[i + 1];
            if (e > total) e = total;  // (never: the offsets are a scan ending in total)
            if (o > e) o = e;
        }
        const uint64_t len = e - o;
        const bool wide = len > kLaneSet;
        const uint64_t m = __ballot(wide);
        if (m) {  // (wave-uniform) the long sets of this wave: one atomic
            const int lane = pad::lane_id(), first = __ffsll((long long)m) - 1;
            unsigned long long at = 0;
            if (lane == first) at = atomicAdd(qcount, (unsigned long long)__popcll(m));
            at = pad::shfl64(at, first);
            if (wide) queue[at + __popcll(m & ((1ull << lane) - 1))] = (uint32_t)i;
        }
        if (i >= n || wide) continue;
        uint32_t node = kNoNode;
        if (len) {
            uint32_t mn = 0xFFFFFFFFu, mx = 0;
            bool ok = true;
            for (uint64_t j = o; j < e; j++) {
                const uint32_t g = sets[j];
                if (g >= t.G) {
                    ok = false;
                    continue;
                }
                const uint32_t x = t.gpre[g];
                mn = min(mn, x), mx = max(mx, x);
            }
            if (ok && mx < t.n_nodes) {
                node = climb(t, mn, mx);
                count_node<LDS>(lineage_hist, direct, node);
            } else {
                atomicOr(err, 1u);
            }
        } else if (type && type[i] == PA_AMBIGUOUSLY_MAPPED) {
            atomicOr(err, 2u);
        }
        node_out[i] = node;
    }
    hist_flush<LDS>(lineage_hist, direct, t.n_nodes);
}

// A wave per queued set: the lanes stride over it (consecutive lanes read
// consecutive genomes), a wave min and max, lane 0 climbs and counts.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_lineage_wave(const uint32_t *__restrict__ queue, uint64_t nq,
                                                         const uint64_t *__restrict__ set_off,
                                                         const uint32_t *__restrict__ sets, uint64_t total, TreeDev t,
                                                         uint32_t *__restrict__ node_out,
                                                         unsigned long long *__restrict__ direct, uint32_t *err) {
    extern __shared__ uint32_t lineage_hist[];
    hist_clear<LDS>(lineage_hist, t.n_nodes);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t q = (uint64_t)blockIdx.x * (kBlock / 64) + wave; q < nq; q += (uint64_t)gridDim.x * (kBlock / 64)) {
        const uint32_t i = queue[q];
        uint64_t o = set_off[i], e = set_off[i + 1];
        if (e > total) e = total;
        if (o > e) o = e;
        uint32_t inv_mn = 0, mx = 0, bad = 0;  // (inv_mn = ~min: both reductions are maxima with identity 0)
        for (uint64_t j = o + lane; j < e; j += 64) {
            const uint32_t g = sets[j];
            if (g >= t.G) {
                bad = 1;
                continue;
            }
            const uint32_t x = t.gpre[g];
            inv_mn = max(inv_mn, ~x), mx = max(mx, x);
        }
        // (all 64 lanes are here: q and the loop bounds are wave-uniform)
        const uint32_t mn = ~pad::wave_max(inv_mn);
        mx = pad::wave_max(mx);
        bad = pad::wave_max(bad);
        if (lane == 0) {
            uint32_t node = kNoNode;
            if (!bad && mn <= mx && mx < t.n_nodes) {
                node = climb(t, mn, mx);
                count_node<LDS>(lineage_hist, direct, node);
            } else {
                atomicOr(err, 1u);
            }
            node_out[i] = node;
        }
    }
    hist_flush<LDS>(lineage_hist, direct, t.n_nodes);
}

inline unsigned grid_for(uint64_t n, unsigned cap) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, cap));
}

// The two kernels over n sets on the device: node_out[n] written, direct (the
// accumulator's, or a scratch array of the caller's) counted.
pa_status reduce_sets(const pa_lineage *l, const uint8_t *d_type, const uint64_t *d_off, const uint32_t *d_sets,
                      uint64_t n, uint64_t total, uint32_t *d_node, unsigned long long *d_direct, pa::Bufs &b,
                      hipStream_t st, const char *what) {
    uint32_t *queue = nullptr, *err = nullptr;
    unsigned long long *qcount = nullptr;
    PA_HIP(b.get(&queue, n * 4));
    PA_HIP(b.get(&qcount, 8));
    PA_HIP(b.get(&err, 4));
    PA_HIP(hipMemsetAsync(qcount, 0, 8, st));
    PA_HIP(hipMemsetAsync(err, 0, 4, st));
    const TreeDev t{l->parent, l->last, l->node_of, l->gpre, l->n_nodes, l->n_genomes};
    // (PA_LINEAGE_LDS=0: global atomics for every tree; read per call, as PA_BOOT_LDS)
    const bool lds = l->n_nodes <= PA_LINEAGE_LDS_NODES && !pa::env_is("PA_LINEAGE_LDS", '0');
    const size_t lds_bytes = lds ? (size_t)l->n_nodes * 4 : 0;
    // a block's uint32 histogram cannot wrap: a batch holds fewer than 2^32 sets
    const unsigned grid = grid_for(n, 2048);
    if (lds)
        hipLaunchKernelGGL(k_lineage_lane<true>, dim3(grid), dim3(kBlock), lds_bytes, st, d_type, d_off, d_sets, n,
                           total, t, d_node, d_direct, queue, qcount, err);
    else
        hipLaunchKernelGGL(k_lineage_lane<false>, dim3(grid), dim3(kBlock), 0, st, d_type, d_off, d_sets, n, total, t,
                           d_node, d_direct, queue, qcount, err);
    PA_HIP(hipGetLastError());
    unsigned long long nq = 0;
    PA_HIP(hipMemcpyAsync(&nq, qcount, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (nq) {
        // a wave per set, 16 sets per wave or more: the histogram's flush is paid per block
        const unsigned gw = grid_for((nq + 15) / 16 * 64, 1024);
        if (lds)
            hipLaunchKernelGGL(k_lineage_wave<true>, dim3(gw), dim3(kBlock), lds_bytes, st, queue, (uint64_t)nq, d_off,
                               d_sets, total, t, d_node, d_direct, err);
        else
            hipLaunchKernelGGL(k_lineage_wave<false>, dim3(gw), dim3(kBlock), 0, st, queue, (uint64_t)nq, d_off, d_sets,
                               total, t, d_node, d_direct, err);
        PA_HIP(hipGetLastError());
    }
    uint32_t h_err = 0;
    PA_HIP(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (h_err & 2u) {
        pa::set_error(std::string(what) + ": an ambiguous read has no candidate genome (invariant violated)");
        return PA_EINTERNAL;
    }
    if (h_err & 1u) {
        pa::set_error(std::string(what) + ": a set holds a genome number outside the index");
        return PA_EINVAL;
    }
    return PA_OK;
}

}  // namespace

namespace pa {

pa_status lineage_create(const pa_index *idx, const uint32_t *parent, uint32_t n_nodes, const uint32_t *genome_node,
                         pa_lineage **out) {
    ErrOp op("pa_lineage_create");
    const uint32_t G = idx->n_genomes;
    if (const char *why = tree_check(parent, n_nodes, genome_node, G)) {
        set_error(std::string("pa_lineage_create: ") + why);
        return PA_EINVAL;
    }
    std::unique_ptr<pa_lineage, void (*)(pa_lineage *)> l(new (std::nothrow) pa_lineage(), lineage_free);
    if (!l) {
        set_error("out of host memory");
        return PA_ENOMEM;
    }
    acc_bind(*l, idx);
    l->n_nodes = n_nodes;
    Preorder t;
    try {
        l->h_parent.assign(parent, parent + n_nodes);
        t = tree_preorder(parent, n_nodes);
        l->h_gpre.resize(G);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory");
        return PA_ENOMEM;
    }
    for (uint32_t g = 0; g < G; g++) l->h_gpre[g] = t.pre[genome_node[g]];
    const uint64_t nb = (uint64_t)n_nodes * 4;
    PA_HIP(pa::dev_malloc(&l->parent, nb));
    PA_HIP(pa::dev_malloc(&l->last, nb));
    PA_HIP(pa::dev_malloc(&l->node_of, nb));
    PA_HIP(pa::dev_malloc(&l->gpre, std::max<uint64_t>((uint64_t)G * 4, 16)));
    PA_HIP(pa::dev_malloc(&l->direct, (uint64_t)n_nodes * 8));
    PA_HIP(pa::dev_malloc(&l->counts, (4 + (uint64_t)G) * 8));
    PA_HIP(hipMemcpy(l->parent, t.parent_pre.data(), nb, hipMemcpyHostToDevice));
    PA_HIP(hipMemcpy(l->last, t.last.data(), nb, hipMemcpyHostToDevice));
    PA_HIP(hipMemcpy(l->node_of, t.node_of.data(), nb, hipMemcpyHostToDevice));
    if (G) PA_HIP(hipMemcpy(l->gpre, l->h_gpre.data(), (uint64_t)G * 4, hipMemcpyHostToDevice));
    PA_HIP(hipMemset(l->direct, 0, (uint64_t)n_nodes * 8));
    PA_HIP(hipMemset(l->counts, 0, (4 + (uint64_t)G) * 8));
    PA_HIP(hipStreamSynchronize(nullptr));
    *out = l.release();
    return PA_OK;
}

void lineage_free(pa_lineage *l) {
    if (!l) return;
    pa::dev_free(l->parent);
    pa::dev_free(l->last);
    pa::dev_free(l->node_of);
    pa::dev_free(l->gpre);
    pa::dev_free(l->direct);
    pa::dev_free(l->counts);
    delete l;
}

pa_status lineage_reset(pa_lineage *l, hipStream_t st) {
    PA_HIP(hipMemsetAsync(l->direct, 0, (uint64_t)l->n_nodes * 8, st));
    PA_HIP(hipMemsetAsync(l->counts, 0, (4 + (uint64_t)l->n_genomes) * 8, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

pa_status lineage_add(pa_index *idx, const pa_reads *r, const DevParams &p, pa_lineage *acc, uint32_t *read_node,
                      hipStream_t st) {
    const uint64_t n = r->n;
    if (n == 0) return PA_OK;
    Bufs b(st);
    CandDev c;
    PA_TRY(candidates_device(idx, r, p, ~0ull, acc->counts, c, b, st));
    uint32_t *d_node = nullptr;
    PA_HIP(b.get(&d_node, n * 4));
    PA_TRY(reduce_sets(acc, c.as.type, c.off, c.sets, n, c.sets ? c.total : 0, d_node, acc->direct, b, st,
                       "pa_lineage_add"));
    if (read_node) {
        PA_HIP(hipMemcpyAsync(read_node, d_node, n * 4, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
    }
    return PA_OK;
}

pa_status lineage_counts(const pa_lineage *l, uint64_t *direct, uint64_t *clade, pa_lineage_info *info,
                         hipStream_t st) {
    const uint32_t n = l->n_nodes;
    std::vector<uint64_t> h(n), cl;
    unsigned long long t[4] = {0, 0, 0, 0};
    PA_HIP(hipMemcpyAsync(h.data(), l->direct, (uint64_t)n * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(t, l->counts, sizeof t, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (direct) std::copy(h.begin(), h.end(), direct);
    if (clade) tree_clade_sums(l->h_parent.data(), n, h.data(), clade);  // O(nodes), on the host
    if (info) {
        info->reads_unique = t[0], info->reads_ambiguous = t[1], info->reads_unmapped = t[2], info->reads_dropped = t[3];
        info->n_nodes = n, info->reserved = 0;
    }
    return PA_OK;
}

pa_status lineage_lca(const pa_lineage *l, const uint64_t *set_off, const uint32_t *sets, uint64_t n_sets,
                      uint32_t *node_out, hipStream_t st) {
    if (n_sets == 0) return PA_OK;
    const uint64_t total = set_off[n_sets];
    Bufs b(st);
    uint64_t *d_off = nullptr;
    uint32_t *d_sets = nullptr, *d_node = nullptr;
    unsigned long long *d_direct = nullptr;  // (counted and thrown away: the accumulator is not touched)
    PA_HIP(b.get(&d_off, (n_sets + 1) * 8));
    PA_HIP(b.get(&d_sets, total * 4));
    PA_HIP(b.get(&d_node, n_sets * 4));
    PA_HIP(b.get(&d_direct, (uint64_t)l->n_nodes * 8));
    PA_HIP(hipMemcpyAsync(d_off, set_off, (n_sets + 1) * 8, hipMemcpyHostToDevice, st));
    if (total) PA_HIP(hipMemcpyAsync(d_sets, sets, total * 4, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemsetAsync(d_direct, 0, (uint64_t)l->n_nodes * 8, st));
    PA_HIP(hipStreamSynchronize(st));  // (the caller's arrays are pageable)
    PA_TRY(reduce_sets(l, nullptr, d_off, d_sets, n_sets, total, d_node, d_direct, b, st, "pa_lineage_lca"));
    PA_HIP(hipMemcpyAsync(node_out, d_node, n_sets * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

}  // namespace pa
