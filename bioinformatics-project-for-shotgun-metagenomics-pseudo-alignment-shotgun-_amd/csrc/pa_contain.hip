// pa_contain.hip -- k-mer containment: which of the reference's distinct k-mers
// the reads hold, counted per genome and per node of a lineage tree.
// DESIGN.md section 21.
//
//   bits       one bit per table slot (a slot is one distinct k-mer), set when a
//              retained window of a read finds that slot.
//   mark       k_contain_mark, a wave per read: the wave packs up to 512 bases of
//              the read to 2 bits in LDS with three ballots per 64 bases (and the
//              qualities' prefix sums beside them), then every lane takes one
//              window of each 64: its key out of the packed words, one ordered
//              probe, a plain load of the bitset word and an atomic OR only when
//              the bit is clear.  No per-read dedup and no per-genome scratch:
//              a repeated k-mer finds its bit set.
//   reduction  k_contain_scan reads every slot once into count[class] and
//              seen[class] (singletons by genome, multi classes by record
//              offset); k_contain_singles / k_contain_classes spread those over
//              the genomes of each class and, with a pa_lineage, add them at the
//              class's node: the min / max preorder number and the climb of
//              pa_tree_dev.h.  Clade sums are host work (pa_tree.h).
//   Integer OR and integer add only: the result does not depend on the batches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <new>

#include "pa_device.h"
#include "pa_internal.h"
#include "pa_tree.h"
#include "pa_tree_dev.h"

using namespace pad;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kChunkW = 256;             // windows per staging of a read
constexpr uint32_t kStage = 512;              // bases staged: kChunkW + k - 1 <= 510 (k <= 255)
constexpr uint32_t kPkWords = kStage / 32 + 2;  // (the key's last load may touch the word after its bits)
constexpr uint32_t kBadWords = kStage / 64 + 2;
constexpr uint32_t F_MRQ = PA_HAS_MIN_READ_QUALITY, F_MKQ = PA_HAS_MIN_KMER_QUALITY, F_MG = PA_HAS_MAX_GENOMES;
// counters of a pa_containment: the seven of pa_containment_info, then the atomic ORs issued
enum { C_READS, C_DROPPED, C_WINDOWS, C_RETAINED, C_FQ, C_FHR, C_ABSENT, C_ISSUED, C_N };

struct MarkArgs {
    const void *table;
    HomeCfg home;
    const uint32_t *class_genomes;
    uint32_t G;
    int k;
    const uint8_t *seq, *qual;
    const uint64_t *off;
    uint64_t n;
    pa::DevParams prm;
    uint32_t *bits;
    unsigned long long *hits, *counters;
};

// The bits of a 32-bit value spread to the even bits of 64.
__device__ __forceinline__ uint64_t spread32(uint64_t x) {
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

// One single-word key, a whole 64-B line (4 slots) per step, ending on the
// ordered clusters' test: probe_lines (pa_device.h) for one key, which also
// says where the key lies -- the bit to set is the slot's number.
__device__ __forceinline__ bool find_line(const Slot<1> *__restrict__ t, const HomeCfg &hc, uint64_t key,
                                          uint64_t &slot, uint32_t &cls) {
    Key<1> kk;
    kk.w[0] = key;
    uint64_t pos = home_of<1>(kk, key_hash(kk), hc);
    for (;;) {
        const uint64_t b = pos & ~3ull;  // (cap % 4 == 0: the line is inside the table)
        // the line as four 16-B loads held in registers: {key lo, key hi, cls, tpos}
        const uint4 *line = reinterpret_cast<const uint4 *>(t + b);
        const uint4 v0 = line[0], v1 = line[1], v2 = line[2], v3 = line[3];
        const uint64_t k0 = ((uint64_t)v0.y << 32) | v0.x, k1 = ((uint64_t)v1.y << 32) | v1.x;
        const uint64_t k2 = ((uint64_t)v2.y << 32) | v2.x, k3 = ((uint64_t)v3.y << 32) | v3.x;
        const uint32_t first = (uint32_t)(pos - b);  // slots before the key's home are not its cluster's
        // the first slot at or after `first` that ends the search: the key, or an empty slot
        uint32_t hit = 4, end = 4;
        if (k3 == key) hit = 3;
        if (k2 == key && first <= 2) hit = 2;
        if (k1 == key && first <= 1) hit = 1;
        if (k0 == key && first == 0) hit = 0;
        if (k3 == EMPTY) end = 3;
        if (k2 == EMPTY && first <= 2) end = 2;
        if (k1 == EMPTY && first <= 1) end = 1;
        if (k0 == EMPTY && first == 0) end = 0;
        if (hit < end) {  // (keys are distinct and never EMPTY: hit != end unless both are 4)
            slot = b + hit;
            cls = cls_of(hit == 0 ? v0.z : hit == 1 ? v1.z : hit == 2 ? v2.z : v3.z);
            return true;
        }
        if (end < 4) return false;
        Key<1> last;
        last.w[0] = k3;
        if (probe_past_key<1>(last, kk, b + 3, hc)) return false;
        pos = (b + 4 == hc.cap) ? 0 : b + 4;
    }
}

template <int NW>
__device__ __forceinline__ bool find_slot(const Slot<NW> *__restrict__ t, const HomeCfg &hc, const Key<NW> &key,
                                          uint64_t &slot, uint32_t &cls) {
    if constexpr (NW == 1) {
        return find_line(t, hc, key.w[0], slot, cls);
    } else {
        uint32_t tpos;
        if (!table_find<NW, true>(t, hc.cap, key, home_of(key, key_hash(key), hc), slot, cls, tpos)) return false;
        cls = cls_of(cls);
        return true;
    }
}

// A wave per read.  LDS: hits_specific through a uint32 histogram of the block
// (G <= PA_LINEAGE_LDS_NODES), else 64-bit global atomics.
template <int NW, bool LDS>
__global__ __launch_bounds__(kBlock) void k_contain_mark(MarkArgs a) {
    extern __shared__ uint32_t contain_hist[];
    __shared__ uint64_t sh_pk[kWaves][kPkWords];    // MSB-first 2-bit words of the staged bases
    __shared__ uint64_t sh_bad[kWaves][kBadWords];  // LSB-first: a base other than ACGT
    __shared__ uint32_t sh_qp[kWaves][kStage + 2];  // qp[i]: the quality sum of the staged bases before i
    __shared__ unsigned long long blk[C_N];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *pk = sh_pk[wave], *bad = sh_bad[wave];
    uint32_t *qp = sh_qp[wave];
    if (LDS) {
        for (uint32_t g = threadIdx.x; g < a.G; g += kBlock) contain_hist[g] = 0;
    }
    if (threadIdx.x < C_N) blk[threadIdx.x] = 0;
    __syncthreads();
    const Slot<NW> *table = (const Slot<NW> *)a.table;
    const int k = a.k;
    const bool has_mrq = a.prm.flags & F_MRQ, has_mkq = a.prm.flags & F_MKQ, has_mg = a.prm.flags & F_MG;
    const uint32_t T = (uint32_t)a.prm.mkq * (uint32_t)k;  // (mkq <= 256, k <= 255)
    uint64_t n_reads = 0, n_drop = 0, n_win = 0;                    // wave-uniform
    uint64_t n_ret = 0, n_fq = 0, n_hr = 0, n_abs = 0, n_iss = 0;   // per lane
    for (uint64_t r = (uint64_t)blockIdx.x * kWaves + wave; r < a.n; r += (uint64_t)gridDim.x * kWaves) {
        const uint64_t off = a.off[r];
        const uint64_t len = a.off[r + 1] - off;
        n_reads++;
        if (has_mrq) {
            uint64_t s = 0;
            for (uint64_t i = lane; i < len; i += 64) s += a.qual[off + i];
            s = wave_sum64(s);
            if ((int64_t)s < (int64_t)a.prm.mrq * (int64_t)len) {
                n_drop++;
                continue;
            }
        }
        const uint64_t W = (k > 0 && len >= (uint64_t)k) ? len - (uint64_t)k + 1 : 0;
        n_win += W;
        for (uint64_t s0 = 0; s0 < W; s0 += kChunkW) {
            const uint32_t cw = W - s0 < kChunkW ? (uint32_t)(W - s0) : kChunkW;
            const uint32_t nb = cw + (uint32_t)k - 1;  // <= kStage - 2, and s0 + nb <= len
            // ---- stage: 64 bases a step, three ballots, the two planes interleaved MSB-first
            uint32_t carry = 0;
            if (lane == 0) qp[0] = 0;
            for (uint32_t b = 0; b < nb; b += 64) {
                const uint32_t i = b + lane;
                const uint32_t c = i < nb ? base_code(a.seq[off + s0 + i]) : 4u;
                const uint64_t lo = __brevll(__ballot(c & 1u)), hi = __brevll(__ballot(c & 2u));
                const uint64_t bd = __ballot(c >= 4u);
                if (lane == 0) {
                    pk[b / 32] = (spread32(hi >> 32) << 1) | spread32(lo >> 32);
                    pk[b / 32 + 1] = (spread32(hi & 0xFFFFFFFFull) << 1) | spread32(lo & 0xFFFFFFFFull);
                    bad[b / 64] = bd;
                }
                if (has_mkq) {
                    const uint32_t q = i < nb ? a.qual[off + s0 + i] : 0u;
                    const uint32_t inc = wave_incl_scan(q) + carry;
                    qp[i + 1] = inc;
                    carry = __shfl(inc, 63);
                }
            }
            wave_sync();
            // ---- windows: a lane takes one of each 64
            for (uint32_t wb = 0; wb < cw; wb += 64) {
                const uint32_t w = wb + lane;
                if (w >= cw) continue;
                if (has_mkq && qp[w + k] - qp[w] < T) {
                    n_fq++;
                    continue;
                }
                if (window_any(bad, w, k)) {
                    n_abs++;
                    continue;
                }
                const Key<NW> key = extract_key<NW>(pk, w, k);
                uint64_t slot;
                uint32_t cls;
                if (!find_slot<NW>(table, a.home, key, slot, cls)) {
                    n_abs++;
                    continue;
                }
                if (has_mg && (int64_t)class_size_of(cls, a.G, a.class_genomes) > (int64_t)a.prm.mg) {
                    n_hr++;
                    continue;
                }
                n_ret++;
                uint32_t *wd = a.bits + (slot >> 5);
                const uint32_t m = 1u << (slot & 31);
                if (!(*wd & m)) {  // a stale 0 only costs the atomic; bits are never cleared by a kernel
                    atomicOr(wd, m);
                    n_iss++;
                }
                if (cls < a.G) {
                    if (LDS)
                        atomicAdd(&contain_hist[cls], 1u);
                    else
                        atomicAdd(&a.hits[cls], 1ull);
                }
            }
            wave_sync();  // (the next staging overwrites what the lanes read)
        }
    }
    // (all 64 lanes are here: the loops' bounds are wave-uniform)
    n_ret = wave_sum64(n_ret), n_fq = wave_sum64(n_fq), n_hr = wave_sum64(n_hr);
    n_abs = wave_sum64(n_abs), n_iss = wave_sum64(n_iss);
    if (lane == 0) {
        atomicAdd(&blk[C_READS], (unsigned long long)n_reads);
        atomicAdd(&blk[C_DROPPED], (unsigned long long)n_drop);
        atomicAdd(&blk[C_WINDOWS], (unsigned long long)n_win);
        atomicAdd(&blk[C_RETAINED], (unsigned long long)n_ret);
        atomicAdd(&blk[C_FQ], (unsigned long long)n_fq);
        atomicAdd(&blk[C_FHR], (unsigned long long)n_hr);
        atomicAdd(&blk[C_ABSENT], (unsigned long long)n_abs);
        atomicAdd(&blk[C_ISSUED], (unsigned long long)n_iss);
    }
    __syncthreads();
    if (threadIdx.x < C_N && blk[threadIdx.x]) atomicAdd(&a.counters[threadIdx.x], blk[threadIdx.x]);
    if (LDS) {
        for (uint32_t g = threadIdx.x; g < a.G; g += kBlock)
            if (contain_hist[g]) atomicAdd(&a.hits[g], (unsigned long long)contain_hist[g]);
    }
}

// Stage A: every slot once.  count / seen: [G + class_entries], a singleton at
// its genome, a multi class at G + its record offset -- the slot's class id.
template <int NW>
__global__ __launch_bounds__(kBlock) void k_contain_scan(const Slot<NW> *__restrict__ table, uint64_t cap, uint32_t G,
                                                         const uint32_t *__restrict__ bits,
                                                         unsigned long long *count, unsigned long long *seen,
                                                         int use_lds) {
    extern __shared__ uint32_t scan_hist[];  // [2 G]: count, seen of the singletons
    if (use_lds) {
        for (uint32_t i = threadIdx.x; i < 2 * G; i += kBlock) scan_hist[i] = 0;
        __syncthreads();
    }
    for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * kBlock) {
        if (table[s].key[0] == EMPTY) continue;
        const uint32_t c = cls_of(table[s].cls);
        const bool on = (bits[s >> 5] >> (s & 31)) & 1u;
        if (c < G && use_lds) {
            atomicAdd(&scan_hist[c], 1u);
            if (on) atomicAdd(&scan_hist[G + c], 1u);
        } else {
            atomicAdd(&count[c], 1ull);
            if (on) atomicAdd(&seen[c], 1ull);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (uint32_t g = threadIdx.x; g < G; g += kBlock) {
            if (scan_hist[g]) atomicAdd(&count[g], (unsigned long long)scan_hist[g]);
            if (scan_hist[G + g]) atomicAdd(&seen[g], (unsigned long long)scan_hist[G + g]);
        }
    }
}

// Stages B for the singletons, a lane per genome: its own k-mers, at its own node.
__global__ __launch_bounds__(kBlock) void k_contain_singles(uint32_t G, const unsigned long long *__restrict__ count,
                                                            const unsigned long long *__restrict__ seen,
                                                            unsigned long long *kmers, unsigned long long *kseen,
                                                            int tree, TreeDev t, unsigned long long *dk,
                                                            unsigned long long *ds) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= G) return;
    const unsigned long long n = count[g], s = seen[g];
    if (!n) return;
    atomicAdd(&kmers[g], n);
    if (s) atomicAdd(&kseen[g], s);
    if (tree) {
        const uint32_t x = t.gpre[g];
        if (x >= t.n_nodes) return;  // (never: pa_lineage_create checked genome_node)
        const uint32_t node = climb(t, x, x);
        atomicAdd(&dk[node], n);
        if (s) atomicAdd(&ds[node], s);
    }
}

// Stages B for the multi classes, a wave per class: B1 adds the class's two
// counts to every genome of its record (the diagonal of k_extsim_classes), B2
// takes the min and max preorder number on the way and adds them at the climb's node.
__global__ __launch_bounds__(kBlock) void k_contain_classes(uint64_t n_cls, const uint64_t *__restrict__ class_off,
                                                            const uint32_t *__restrict__ class_size,
                                                            const uint32_t *__restrict__ class_genomes, uint32_t G,
                                                            const unsigned long long *__restrict__ count,
                                                            const unsigned long long *__restrict__ seen,
                                                            unsigned long long *kmers, unsigned long long *kseen,
                                                            int tree, TreeDev t, unsigned long long *dk,
                                                            unsigned long long *ds) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t c = (uint64_t)blockIdx.x * kWaves + wave; c < n_cls; c += (uint64_t)gridDim.x * kWaves) {
        const uint64_t o = class_off[c];
        const unsigned long long n = count[G + o], s = seen[G + o];
        if (!n) continue;  // (wave-uniform)
        const uint32_t sz = class_size[c];
        const uint32_t *gl = class_genomes + o + 1;
        uint32_t inv_mn = 0, mx = 0;  // (inv_mn = ~min: both reductions are maxima with identity 0)
        for (uint32_t j = lane; j < sz; j += 64) {
            const uint32_t g = gl[j];
            if (g >= G) continue;  // (never: the build wrote the record)
            atomicAdd(&kmers[g], n);
            if (s) atomicAdd(&kseen[g], s);
            if (tree) {
                const uint32_t x = t.gpre[g];
                inv_mn = max(inv_mn, ~x), mx = max(mx, x);
            }
        }
        if (tree) {
            const uint32_t mn = ~wave_max(inv_mn);
            mx = wave_max(mx);
            if (lane == 0 && mn <= mx && mx < t.n_nodes) {
                const uint32_t node = climb(t, mn, mx);
                atomicAdd(&dk[node], n);
                if (s) atomicAdd(&ds[node], s);
            }
        }
    }
}

template <int NW>
void launch_mark(const MarkArgs &a, bool lds, unsigned grid, hipStream_t st) {
    if (lds)
        hipLaunchKernelGGL((k_contain_mark<NW, true>), dim3(grid), dim3(kBlock), (size_t)a.G * 4, st, a);
    else
        hipLaunchKernelGGL((k_contain_mark<NW, false>), dim3(grid), dim3(kBlock), 0, st, a);
}

template <int NW>
void launch_scan(const pa_containment *c, unsigned long long *count, unsigned long long *seen, hipStream_t st) {
    const pa_index *idx = c->idx;
    // a block's uint32 histogram cannot wrap: 4096 blocks share the slots of a table (< 2^44)
    const int use_lds = idx->n_genomes <= PA_LINEAGE_LDS_NODES;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((idx->cap + kBlock - 1) / kBlock, 4096));
    hipLaunchKernelGGL(k_contain_scan<NW>, dim3(grid), dim3(kBlock), use_lds ? (size_t)idx->n_genomes * 8 : 0, st,
                       (const Slot<NW> *)idx->table, idx->cap, idx->n_genomes, c->bits, count, seen, use_lds);
}

// The reduction: host vectors kmers, kmers_seen, specific, specific_seen [G]
// and, with a lineage, direct_kmers and direct_seen [n_nodes].
struct Reduced {
    std::vector<uint64_t> kmers, kseen, spec, sseen, dk, ds;
};
pa_status reduce(const pa_containment *c, const pa_lineage *l, Reduced &out, hipStream_t st) {
    const pa_index *idx = c->idx;
    const uint32_t G = idx->n_genomes;
    const uint64_t n_cls = (uint64_t)G + idx->class_entries;
    const uint32_t nn = l ? l->n_nodes : 0;
    try {
        out.kmers.assign(G, 0), out.kseen.assign(G, 0), out.spec.assign(G, 0), out.sseen.assign(G, 0);
        out.dk.assign(nn, 0), out.ds.assign(nn, 0);
    } catch (const std::bad_alloc &) {
        pa::set_error("out of host memory");
        return PA_ENOMEM;
    }
    if (idx->n_kmers == 0 || G == 0) return PA_OK;
    pa::Bufs b(st);
    unsigned long long *count = nullptr, *seen = nullptr, *kmers = nullptr, *kseen = nullptr, *dk = nullptr,
                       *ds = nullptr;
    PA_HIP(b.get(&count, n_cls * 8));
    PA_HIP(b.get(&seen, n_cls * 8));
    PA_HIP(b.get(&kmers, (uint64_t)G * 8));
    PA_HIP(b.get(&kseen, (uint64_t)G * 8));
    PA_HIP(hipMemsetAsync(count, 0, n_cls * 8, st));
    PA_HIP(hipMemsetAsync(seen, 0, n_cls * 8, st));
    PA_HIP(hipMemsetAsync(kmers, 0, (uint64_t)G * 8, st));
    PA_HIP(hipMemsetAsync(kseen, 0, (uint64_t)G * 8, st));
    TreeDev t{nullptr, nullptr, nullptr, nullptr, 0, G};
    if (l) {
        PA_HIP(b.get(&dk, (uint64_t)nn * 8));
        PA_HIP(b.get(&ds, (uint64_t)nn * 8));
        PA_HIP(hipMemsetAsync(dk, 0, (uint64_t)nn * 8, st));
        PA_HIP(hipMemsetAsync(ds, 0, (uint64_t)nn * 8, st));
        t = TreeDev{l->parent, l->last, l->node_of, l->gpre, l->n_nodes, G};
    }
    pa::with_nw(idx->nw, [&](auto w) { launch_scan<w()>(c, count, seen, st); });
    PA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_contain_singles, dim3((G + kBlock - 1) / kBlock), dim3(kBlock), 0, st, G, count, seen, kmers,
                       kseen, l ? 1 : 0, t, dk, ds);
    PA_HIP(hipGetLastError());
    if (idx->n_multi) {
        const unsigned grid = (unsigned)std::min<uint64_t>((idx->n_multi + kWaves - 1) / kWaves, 2048);
        hipLaunchKernelGGL(k_contain_classes, dim3(grid), dim3(kBlock), 0, st, idx->n_multi, idx->class_off,
                           idx->class_size, idx->class_genomes, G, count, seen, kmers, kseen, l ? 1 : 0, t, dk, ds);
        PA_HIP(hipGetLastError());
    }
    PA_HIP(hipMemcpyAsync(out.kmers.data(), kmers, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(out.kseen.data(), kseen, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(out.spec.data(), count, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(out.sseen.data(), seen, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    if (l) {
        PA_HIP(hipMemcpyAsync(out.dk.data(), dk, (uint64_t)nn * 8, hipMemcpyDeviceToHost, st));
        PA_HIP(hipMemcpyAsync(out.ds.data(), ds, (uint64_t)nn * 8, hipMemcpyDeviceToHost, st));
    }
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

inline uint64_t hits_bytes(uint32_t G) { return std::max<uint64_t>((uint64_t)G * 8, 16); }

}  // namespace

namespace pa {

pa_status containment_create(const pa_index *idx, pa_containment **out) {
    ErrOp op("pa_containment_create");
    std::unique_ptr<pa_containment, void (*)(pa_containment *)> c(new (std::nothrow) pa_containment(),
                                                                  containment_free);
    if (!c) {
        set_error("out of host memory");
        return PA_ENOMEM;
    }
    acc_bind(*c, idx);
    c->bits_bytes = std::max<uint64_t>((idx->cap + 31) / 32 * 4, 16);  // cap / 8, whole 32-bit words
    PA_HIP(pa::dev_malloc(&c->bits, c->bits_bytes));
    PA_HIP(pa::dev_malloc(&c->hits, hits_bytes(idx->n_genomes)));
    PA_HIP(pa::dev_malloc(&c->counters, C_N * 8));
    PA_TRY(containment_reset(c.get(), nullptr));
    *out = c.release();
    return PA_OK;
}

void containment_free(pa_containment *c) {
    if (!c) return;
    pa::dev_free(c->bits);
    pa::dev_free(c->hits);
    pa::dev_free(c->counters);
    delete c;
}

pa_status containment_reset(pa_containment *c, hipStream_t st) {
    PA_HIP(hipMemsetAsync(c->bits, 0, c->bits_bytes, st));
    PA_HIP(hipMemsetAsync(c->hits, 0, hits_bytes(c->n_genomes), st));
    PA_HIP(hipMemsetAsync(c->counters, 0, C_N * 8, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

pa_status containment_add(const pa_index *idx, const pa_reads *r, const DevParams &p, pa_containment *acc,
                          hipStream_t st) {
    if (r->n == 0) return PA_OK;
    MarkArgs a{};
    a.table = idx->table, a.home = idx->home, a.class_genomes = idx->class_genomes, a.G = idx->n_genomes;
    a.k = (int)idx->k;
    a.seq = r->seq, a.qual = r->qual, a.off = r->off, a.n = r->n;
    a.prm = p;
    a.bits = acc->bits, a.hits = acc->hits, a.counters = acc->counters;
    // a block's uint32 histogram cannot wrap below 2^32 bases a batch
    const bool lds = idx->n_genomes <= PA_LINEAGE_LDS_NODES && r->n_bases < (1ull << 32) &&
                     !env_is("PA_CONTAIN_LDS", '0');
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((r->n + kWaves - 1) / kWaves, 4096));
    with_nw(idx->nw, [&](auto w) { launch_mark<w()>(a, lds, grid, st); });
    PA_HIP(hipGetLastError());
    PA_HIP(hipStreamSynchronize(st));
    if (env_is("PA_CONTAIN_STATS", '1')) {  // the atomics issued so far, beside the windows retained
        unsigned long long h[C_N];
        PA_HIP(hipMemcpy(h, acc->counters, sizeof h, hipMemcpyDeviceToHost));
        fprintf(stderr, "[pa_contain] windows %llu retained %llu atomic ORs issued %llu (since the last reset)\n",
                h[C_WINDOWS], h[C_RETAINED], h[C_ISSUED]);
    }
    return PA_OK;
}

pa_status containment_counts(const pa_containment *c, uint64_t *kmers, uint64_t *kmers_seen, uint64_t *specific,
                             uint64_t *specific_seen, uint64_t *hits_specific, pa_containment_info *info,
                             hipStream_t st) {
    const uint32_t G = c->n_genomes;
    if (kmers || kmers_seen || specific || specific_seen) {
        Reduced red;
        PA_TRY(reduce(c, nullptr, red, st));
        if (kmers) std::copy(red.kmers.begin(), red.kmers.end(), kmers);
        if (kmers_seen) std::copy(red.kseen.begin(), red.kseen.end(), kmers_seen);
        if (specific) std::copy(red.spec.begin(), red.spec.end(), specific);
        if (specific_seen) std::copy(red.sseen.begin(), red.sseen.end(), specific_seen);
    }
    if (hits_specific && G) PA_HIP(hipMemcpyAsync(hits_specific, c->hits, (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    unsigned long long h[C_N] = {};
    if (info) PA_HIP(hipMemcpyAsync(h, c->counters, sizeof h, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (info) {
        info->reads = h[C_READS], info->reads_dropped = h[C_DROPPED], info->windows = h[C_WINDOWS];
        info->windows_retained = h[C_RETAINED], info->windows_filtered_quality = h[C_FQ];
        info->windows_filtered_hr = h[C_FHR], info->windows_absent = h[C_ABSENT];
    }
    return PA_OK;
}

pa_status containment_nodes(const pa_containment *c, const pa_lineage *l, uint64_t *direct_kmers,
                            uint64_t *direct_seen, uint64_t *clade_kmers, uint64_t *clade_seen, hipStream_t st) {
    Reduced red;
    PA_TRY(reduce(c, l, red, st));
    const uint32_t n = l->n_nodes;
    if (direct_kmers) std::copy(red.dk.begin(), red.dk.end(), direct_kmers);
    if (direct_seen) std::copy(red.ds.begin(), red.ds.end(), direct_seen);
    if (clade_kmers) tree_clade_sums(l->h_parent.data(), n, red.dk.data(), clade_kmers);  // O(nodes), on the host
    if (clade_seen) tree_clade_sums(l->h_parent.data(), n, red.ds.data(), clade_seen);
    return PA_OK;
}

}  // namespace pa
