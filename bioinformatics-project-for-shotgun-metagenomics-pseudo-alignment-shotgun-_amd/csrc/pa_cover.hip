// pa_cover.hip -- per-genome read coverage (depth and breadth): where on a
// genome the reads mapped to it fall.  The course project's EXTCOVERAGE
// extension (--coverage, --genomes, --min-coverage, --full-coverage), which the
// reference leaves out; DESIGN.md section 10 holds the definition.
//
// Three pieces:
//
//   the positions view   for a k-mer found in the table and a genome g of its
//                  set, min(occ(w, g)): the k-mer's first occurrence in g.  Made
//                  with pa_dump.hip's recipe -- K[t] = first position of the
//                  k-mer at window t, a stable radix sort of (K, t) -- of which
//                  only the first element of every (k-mer, genome) run is kept:
//                  cov_first, k-mer after k-mer, genomes ascending inside one.
//                  That is the order of the k-mer's class record, so the entry
//                  of genome g is cov_head[slot] + (rank of g in the record):
//                  one load, whatever the k-mer's occurrences elsewhere.  The
//                  view does not use slot.tpos (made by the tiles, for k <= 63
//                  only) and so serves every k up to PA_MAX_K.
//   k_place        one wave64 per (read, listed genome): lanes take the windows
//                  j = lane, lane + 64, ..., look their k-mers up, form the
//                  diagonals first - j, and the wave takes their mode (smallest
//                  on a tie); lane 0 adds the read's interval(s) to the
//                  genome's difference array.
//   scans          depth = inclusive scan of the difference arrays (every
//                  genome's entries sum to zero, so one scan over all of them
//                  is the segmented one), summaries by one block per genome.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <string>
#include <vector>

#include "pa_device.h"
#include "pa_internal.h"

using namespace pad;

namespace {

constexpr int kBlock = 256;
constexpr int kRun = 16;  // windows per thread in the genome scans
constexpr int64_t kNoDiag = INT64_MIN;

inline unsigned grid_for(uint64_t n, unsigned block = kBlock) {
    uint64_t g = (n + block - 1) / block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, 65536));
}

__global__ void k_fill32(uint32_t *p, uint64_t n, uint32_t v) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

__global__ void k_iota32(uint32_t *p, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        p[i] = (uint32_t)i;
}

// The genome whose region holds concatenated position t (t < goff[G]).
__device__ __forceinline__ uint32_t genome_at(const uint64_t *__restrict__ goff, uint32_t G, uint64_t t) {
    uint32_t lo = 0, hi = G;  // goff[lo] <= t < goff[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (goff[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ---- the positions view ----------------------------------------------------------

// Pass 1 (KEYS = false): fp[slot] = the smallest window position holding the
// slot's k-mer.  Pass 2 (KEYS = true): K[t] = fp of the k-mer at window t.
template <int NW, bool KEYS>
__global__ __launch_bounds__(kBlock) void k_view_scan(const uint8_t *__restrict__ codes, uint64_t gstart, uint64_t nwin,
                                                      int k, uint64_t mask0, const Slot<NW> *__restrict__ table,
                                                      HomeCfg hc, uint32_t *fp, uint32_t *K,
                                                      unsigned long long *n_valid) {
    const uint64_t w0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kRun;
    uint32_t cnt = 0;
    if (w0 < nwin) {
        const uint64_t w1 = min(w0 + (uint64_t)kRun, nwin);
        const uint8_t *s = codes + gstart + w0;
        Key<NW> key;
#pragma unroll
        for (int j = 0; j < NW; j++) key.w[j] = 0;
        int run = 0;
        for (int i = 0; i < k - 1; i++) {
            const uint32_t c = s[i];
            run = c > 3 ? 0 : run + 1;
            key_push(key, c & 3, mask0);
        }
        for (uint64_t w = w0; w < w1; w++) {
            const uint32_t c = s[w - w0 + k - 1];
            run = c > 3 ? 0 : run + 1;
            key_push(key, c & 3, mask0);
            if (run < k) continue;  // (N windows are not indexed, src/kmer.py:145)
            uint64_t slot;
            uint32_t cls, tpos;
            if (!table_find<NW, true>(table, hc.cap, key, home_of(key, key_hash(key), hc), slot, cls, tpos)) continue;
            const uint32_t t = (uint32_t)(gstart + w);
            if constexpr (KEYS) {
                K[t] = fp[slot];
                cnt++;
            } else {
                if (fp[slot] > t) atomicMin(&fp[slot], t);  // (a stale plain load only costs an atomic)
            }
        }
    }
    if constexpr (KEYS) {
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_valid, (unsigned long long)cnt);
    }
}

// flag[i] = 1 where sorted element i is the first of its (k-mer, genome) run.
__global__ void k_view_flags(const uint32_t *__restrict__ K, const uint32_t *__restrict__ T, uint64_t n,
                             const uint64_t *__restrict__ goff, uint32_t G, uint32_t *flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || K[i] != K[i - 1] || genome_at(goff, G, T[i]) != genome_at(goff, G, T[i - 1])) ? 1u : 0u;
}

// The kept elements to cov_first; a k-mer's first element (its first occurrence
// over all genomes: T == K) also names the k-mer's entry in its slot.
template <int NW>
__global__ void k_view_scatter(const uint32_t *__restrict__ K, const uint32_t *__restrict__ T,
                               const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint64_t n,
                               const uint8_t *__restrict__ codes, int k, uint64_t mask0,
                               const Slot<NW> *__restrict__ table, HomeCfg hc, uint32_t *first, uint64_t n_pairs,
                               uint32_t *head, unsigned long long *err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint32_t t = T[i], rk = rank[i];
    if (rk >= n_pairs) {
        atomicAdd(err, 1ull);
        return;
    }
    first[rk] = t;
    if (K[i] != t) return;
    Key<NW> key;
#pragma unroll
    for (int j = 0; j < NW; j++) key.w[j] = 0;
    for (int q = 0; q < k; q++) key_push(key, codes[(uint64_t)t + q] & 3u, mask0);
    uint64_t slot;
    uint32_t cls, tpos;
    if (!table_find<NW, true>(table, hc.cap, key, home_of(key, key_hash(key), hc), slot, cls, tpos)) {
        atomicAdd(err, 1ull);
        return;
    }
    head[slot] = rk;
}

template <int NW>
pa_status view_build(pa_index *idx, hipStream_t st) {
    pa::ErrOp op("pa_index_prepare_coverage");
    pa::Bufs b(st);
    const uint32_t G = idx->n_genomes;
    const uint64_t total = idx->h_goff[G];
    const int k = (int)idx->k;
    const uint64_t mask0 = [&] {
        const int bits = 2 * k - 64 * (NW - 1);
        return bits >= 64 ? ~0ull : ((1ull << bits) - 1);
    }();
    uint32_t *head = nullptr, *first = nullptr, *K = nullptr, *K2 = nullptr, *V = nullptr, *V2 = nullptr;
    unsigned long long *d_n = nullptr;  // [0] valid windows, [1] errors
    const Slot<NW> *table = (const Slot<NW> *)idx->table;
    PA_HIP(b.get(&head, std::max<uint64_t>(idx->cap, 1) * 4));
    PA_HIP(b.get(&K, total * 4));
    PA_HIP(b.get(&K2, total * 4));
    PA_HIP(b.get(&V, total * 4));
    PA_HIP(b.get(&V2, total * 4));
    PA_HIP(b.get(&d_n, 16));
    PA_HIP(hipMemsetAsync(d_n, 0, 16, st));
    hipLaunchKernelGGL(k_fill32, dim3(grid_for(idx->cap)), dim3(kBlock), 0, st, head, idx->cap, NONE);
    hipLaunchKernelGGL(k_fill32, dim3(grid_for(total)), dim3(kBlock), 0, st, K, total, NONE);
    hipLaunchKernelGGL(k_iota32, dim3(grid_for(total)), dim3(kBlock), 0, st, V, total);
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t g = 0; g < G; g++) {
            const uint64_t len = idx->h_goff[g + 1] - idx->h_goff[g];
            if ((uint64_t)k > len) continue;
            const uint64_t nwin = len - k + 1;
            const unsigned grid = (unsigned)(((nwin + kRun - 1) / kRun + kBlock - 1) / kBlock);
            if (pass == 0)
                hipLaunchKernelGGL((k_view_scan<NW, false>), dim3(grid), dim3(kBlock), 0, st, idx->codes, idx->h_goff[g],
                                   nwin, k, mask0, table, idx->home, head, (uint32_t *)nullptr,
                                   (unsigned long long *)nullptr);
            else
                hipLaunchKernelGGL((k_view_scan<NW, true>), dim3(grid), dim3(kBlock), 0, st, idx->codes, idx->h_goff[g],
                                   nwin, k, mask0, table, idx->home, head, K, d_n);
        }
    PA_HIP(hipGetLastError());
    // (positions are < 2^32 - 1, so NONE sorts the windows without a k-mer to the end)
    rocprim::double_buffer<uint32_t> kb(K, K2), vb(V, V2);
    PA_HIP(pa::with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::radix_sort_pairs(tmp, tmp_bytes, kb, vb, total, 0, 32, st);
    }));
    unsigned long long nv = 0;
    PA_HIP(hipMemcpyAsync(&nv, d_n, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    uint64_t n_pairs = 0;
    if (nv) {
        uint32_t *flag = kb.alternate(), *rank = vb.alternate();
        hipLaunchKernelGGL(k_view_flags, dim3((unsigned)((nv + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           kb.current(), vb.current(), (uint64_t)nv, idx->goff, G, flag);
        PA_HIP(hipGetLastError());
        PA_HIP(pa::with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
            return rocprim::exclusive_scan(tmp, tmp_bytes, flag, rank, 0u, (size_t)nv, rocprim::plus<uint32_t>(), st);
        }));
        uint32_t last_rank = 0, last_flag = 0;
        PA_HIP(hipMemcpyAsync(&last_rank, rank + (nv - 1), 4, hipMemcpyDeviceToHost, st));
        PA_HIP(hipMemcpyAsync(&last_flag, flag + (nv - 1), 4, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
        n_pairs = (uint64_t)last_rank + last_flag;
        PA_HIP(b.get(&first, std::max<uint64_t>(n_pairs, 1) * 4));
        // (every occupied slot is some window's k-mer: its fp is overwritten by its entry)
        hipLaunchKernelGGL(k_view_scatter<NW>, dim3((unsigned)((nv + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           kb.current(), vb.current(), flag, rank, (uint64_t)nv, idx->codes, k, mask0, table, idx->home,
                           first, n_pairs, head, d_n + 1);
        PA_HIP(hipGetLastError());
        unsigned long long errs = 0;
        PA_HIP(hipMemcpyAsync(&errs, d_n + 1, 8, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
        if (errs) {
            pa::set_error("pa_index_prepare_coverage: a genome window's k-mer is missing from the table");
            return PA_EINTERNAL;
        }
    }
    idx->cov_head = b.release(head);  // the view outlives the call: the index owns it now
    idx->cov_first = b.release(first);
    idx->cov_pairs = n_pairs;
    idx->cov_bytes = std::max<uint64_t>(idx->cap, 1) * 4 + (first ? std::max<uint64_t>(n_pairs, 1) * 4 : 0);
    idx->device_bytes += idx->cov_bytes;
    idx->cov_ready = 1;
    return PA_OK;
}

// ---- placement -----------------------------------------------------------------

struct PlaceArgs {
    const void *table;
    uint64_t cap;
    HomeCfg home;
    uint32_t G;
    int k;
    const uint32_t *class_genomes;
    const uint64_t *class_mask;  // G <= 64: the sets' membership masks, indexed like class_genomes (else null)
    const uint64_t *goff;
    const uint32_t *head, *first;
    uint64_t n_pairs;
    const uint8_t *seq;
    const uint64_t *off;
    uint64_t n_reads;
    const uint8_t *type;
    const uint64_t *list_off;
    const uint32_t *lists;
    uint64_t n_entries;
    int64_t *starts;           // [n_entries] (nullable)
    uint8_t *agree;            // [n_entries] (nullable): 1 where every voting window named the placement's diagonal
    uint32_t *diff;            // the accumulator (nullable): unique category, the ambiguous one `entries` further
    uint64_t entries;
    const uint64_t *foff;      // forward bases before genome g
    int both;
    int64_t *ws;               // [waves][rounds * 64] the lanes' diagonals
    uint32_t rounds;
    unsigned long long *err;   // [0] listed genomes no window voted for, [1] view entries out of range
};

// +1 over the forward positions [x0, x1) of a genome whose difference entries start at d.
__device__ __forceinline__ void add_interval(uint32_t *d, int64_t x0, int64_t x1) {
    if (x0 >= x1) return;
    atomicAdd(&d[x0], 1u);
    atomicSub(&d[x1], 1u);
}

template <int NW>
__global__ __launch_bounds__(kBlock) void k_place(PlaceArgs a) {
    const int lane = lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    int64_t *my = a.ws + wave * ((uint64_t)a.rounds * 64) + lane;  // window lane + 64 t at my[64 t]
    const Slot<NW> *table = (const Slot<NW> *)a.table;
    const int k = a.k;
    const uint64_t mask0 = mask0_of(k, NW);
    const uint32_t G = a.G;
    for (uint64_t e = wave; e < a.n_entries; e += n_waves) {
        // the read of list entry e: list_off[r] <= e < list_off[r + 1]
        uint64_t lo = 0, hi = a.n_reads;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.list_off[mid] <= e)
                lo = mid;
            else
                hi = mid;
        }
        const uint64_t r = lo;
        const uint32_t g = a.lists[e];
        if (g >= G) {  // (never: the lists hold genome numbers)
            if (lane == 0) atomicAdd(&a.err[1], 1ull);
            continue;
        }
        const uint64_t off = a.off[r];
        const uint32_t len = (uint32_t)(a.off[r + 1] - off);
        const uint32_t W = len >= (uint32_t)k ? len - k + 1 : 0;
        const uint32_t rounds = min((W + 63) / 64, a.rounds);  // (W <= 64 a.rounds: the batch's longest read sized it)
        const uint64_t gs = a.goff[g], rlen = a.goff[g + 1] - gs;
        // ---- the windows' diagonals
        uint32_t votes = 0;
        for (uint32_t t = 0; t < rounds; t++) {
            const uint32_t j = t * 64 + lane;
            int64_t d = kNoDiag;
            if (j < W) {
                Key<NW> key;
#pragma unroll
                for (int q = 0; q < NW; q++) key.w[q] = 0;
                bool clean = true;
                for (int i = 0; i < k; i++) {
                    const uint32_t c = base_code(a.seq[off + j + i]);
                    clean &= c < 4;
                    key_push(key, c & 3, mask0);
                }
                uint64_t slot;
                uint32_t cls, tpos;
                if (clean && table_find<NW, true>(table, a.cap, key, home_of(key, key_hash(key), a.home), slot, cls, tpos)) {
                    // the rank of g in the k-mer's genome set (records are [size, ascending genomes...])
                    const uint32_t c = cls_of(cls);
                    bool member;
                    uint32_t rank = 0;
                    if (c < G) {
                        member = c == g;
                    } else if (a.class_mask) {
                        const uint64_t m = a.class_mask[c - G];
                        member = (m >> g) & 1ull;
                        rank = (uint32_t)__popcll(m & ((1ull << g) - 1));
                    } else {
                        const uint32_t *rec = a.class_genomes + (c - G);
                        const uint32_t sz = rec[0];
                        uint32_t l = 0, h = sz;
                        while (l < h) {
                            const uint32_t mid = l + (h - l) / 2;
                            if (rec[1 + mid] < g)
                                l = mid + 1;
                            else
                                h = mid;
                        }
                        rank = l;
                        member = l < sz && rec[1 + l] == g;
                    }
                    if (member) {
                        const uint64_t ent = (uint64_t)a.head[slot] + rank;
                        if (ent < a.n_pairs) {
                            const uint64_t p = a.first[ent];
                            if (p >= gs && p < gs + rlen)
                                d = (int64_t)(p - gs) - (int64_t)j;
                            else
                                atomicAdd(&a.err[1], 1ull);
                        } else {
                            atomicAdd(&a.err[1], 1ull);
                        }
                    }
                }
            }
            my[64 * t] = d;
            votes += (uint32_t)__popcll(__ballot(d != kNoDiag));
        }
        // ---- their mode, the smallest on a tie: the first window left names a
        // diagonal, the wave counts and removes its windows, until those left
        // could not outvote the best
        uint32_t left = votes, best_cnt = 0;
        int64_t best = 0;
        while (left > 0 && left >= best_cnt) {
            int64_t cand = 0;
            for (uint32_t t = 0; t < rounds; t++) {
                const int64_t d = my[64 * t];
                const uint64_t b = __ballot(d != kNoDiag);
                if (b) {
                    cand = (int64_t)shfl64((uint64_t)d, __ffsll((long long)b) - 1);
                    break;
                }
            }
            uint32_t cnt = 0;
            for (uint32_t t = 0; t < rounds; t++) {
                const bool m = my[64 * t] == cand;
                cnt += (uint32_t)__popcll(__ballot(m));
                if (m) my[64 * t] = kNoDiag;
            }
            if (cnt > best_cnt || (cnt == best_cnt && cand < best)) {
                best_cnt = cnt;
                best = cand;
            }
            left -= cnt;
        }
        if (lane == 0) {
            if (votes == 0) {  // (a listed genome holds a k-mer of the read: never silent)
                atomicAdd(&a.err[0], 1ull);
                best = 0;
            }
            if (a.starts) a.starts[e] = best;
            if (a.agree) a.agree[e] = best_cnt == votes && votes != 0;
            const uint64_t e0 = a.list_off[r];
            // (a p-demoted list holds G* twice: it counts once)
            if (a.diff && votes != 0 && !(e > e0 && a.lists[e0] == g)) {
                uint32_t *dg = a.diff + (a.type[r] == PA_UNIQUELY_MAPPED ? 0 : a.entries) + a.foff[g] + g;
                const int64_t q0 = max(best, (int64_t)0), q1 = min(best + (int64_t)len, (int64_t)rlen);
                if (!a.both) {
                    add_interval(dg, q0, q1);
                } else {
                    // region = g + N + reverse complement: q < |g| is x = q, q > |g| is x = 2|g| - q
                    const int64_t fl = (int64_t)(a.foff[g + 1] - a.foff[g]);
                    add_interval(dg, q0, min(q1, fl));
                    const int64_t qb = max(q0, fl + 1);
                    if (qb < q1) add_interval(dg, 2 * fl - q1 + 1, 2 * fl - qb + 1);
                }
            }
        }
    }
}

template <int NW>
void launch_place(const PlaceArgs &a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL(k_place<NW>, dim3(grid), dim3(kBlock), 0, st, a);
}

// ---- depth and summaries ---------------------------------------------------------

// One block per (genome, category): positions with depth >= minc, and the depths' sum.
__global__ __launch_bounds__(kBlock) void k_cover_summary(const uint32_t *__restrict__ depth, uint64_t entries,
                                                          const uint64_t *__restrict__ foff, uint32_t G, uint32_t minc,
                                                          unsigned long long *out /* [4 G]: covered u, a; sum u, a */) {
    __shared__ unsigned long long red[2][kBlock / 64];
    const uint32_t g = blockIdx.x % G, cat = blockIdx.x / G;
    const uint32_t *d = depth + (uint64_t)cat * entries + foff[g] + g;
    const uint64_t n = foff[g + 1] - foff[g];
    uint64_t cv = 0, sm = 0;
    for (uint64_t x = threadIdx.x; x < n; x += kBlock) {
        const uint32_t v = d[x];
        cv += v >= minc;
        sm += v;
    }
    cv = wave_sum64(cv);
    sm = wave_sum64(sm);
    if (lane_id() == 0) {
        red[0][threadIdx.x >> 6] = cv;
        red[1][threadIdx.x >> 6] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t c = 0, s = 0;
        for (int i = 0; i < kBlock / 64; i++) {
            c += red[0][i];
            s += red[1][i];
        }
        out[(uint64_t)cat * G + g] = c;
        out[(uint64_t)(2 + cat) * G + g] = s;
    }
}

}  // namespace

namespace pa {

void index_release_coverage(pa_index *idx) {
    pa::dev_free(idx->cov_head);
    pa::dev_free(idx->cov_first);
    idx->cov_head = idx->cov_first = nullptr;
    if (idx->cov_ready && idx->device_bytes >= idx->cov_bytes) idx->device_bytes -= idx->cov_bytes;
    idx->cov_pairs = idx->cov_bytes = 0;
    idx->cov_ready = 0;
}

pa_status index_prepare_coverage(pa_index *idx, hipStream_t st) {
    if (idx->cov_ready) return PA_OK;
    const uint64_t total = idx->h_goff.empty() ? 0 : idx->h_goff[idx->n_genomes];
    if (total >= 0xFFFFFFFFull) {
        set_error("coverage needs a reference of fewer than 2^32 region positions (a both-strand index holds "
                  "2 |g| + 1 per genome)");
        return PA_EUNSUPPORTED;
    }
    if (idx->k <= 0 || idx->n_kmers == 0 || total == 0) {  // no k-mer, so no read is ever placed
        idx->cov_ready = 1;
        return PA_OK;
    }
    if (idx->nw < 1 || idx->nw > 8) {
        set_error("unsupported k");
        return PA_EUNSUPPORTED;
    }
    return with_nw(idx->nw, [&](auto w) { return view_build<w()>(idx, st); });
}

pa_status coverage_create(const pa_index *idx, pa_coverage **out) {
    ErrOp op("pa_coverage_create");
    const uint32_t G = idx->n_genomes;
    std::unique_ptr<pa_coverage, void (*)(pa_coverage *)> c(new (std::nothrow) pa_coverage(), coverage_free);
    if (!c) {
        set_error("out of host memory");
        return PA_ENOMEM;
    }
    acc_bind(*c, idx);
    c->h_foff = forward_offsets(idx);
    c->entries = c->h_foff[G] + G;
    PA_HIP(pa::dev_malloc(&c->foff, (uint64_t)(G + 1) * 8));
    PA_HIP(pa::dev_malloc(&c->diff, std::max<uint64_t>(2 * c->entries, 1) * 4));
    PA_HIP(hipMemcpy(c->foff, c->h_foff.data(), (uint64_t)(G + 1) * 8, hipMemcpyHostToDevice));
    PA_HIP(hipMemset(c->diff, 0, std::max<uint64_t>(2 * c->entries, 1) * 4));
    // (a device memset returns before it is done, and the first add may come on a
    // stream that does not wait for the null stream: the zeroes are there on return)
    PA_HIP(hipStreamSynchronize(nullptr));
    *out = c.release();
    return PA_OK;
}

void coverage_free(pa_coverage *cov) {
    if (!cov) return;
    pa::dev_free(cov->foff);
    pa::dev_free(cov->diff);
    pa::dev_free(cov->depth);
    delete cov;
}

pa_status coverage_reset(pa_coverage *cov, hipStream_t st) {
    PA_HIP(hipMemsetAsync(cov->diff, 0, std::max<uint64_t>(2 * cov->entries, 1) * 4, st));
    cov->depth_valid = 0;
    cov->reads_added = 0;
    return PA_OK;
}

pa_status place_device(pa_index *idx, const pa_reads *r, const DevParams &p, pa_coverage *acc,
                       uint64_t list_cap, bool want_starts, bool want_agree, PlacedDev &out, Bufs &b, hipStream_t st) {
    out = PlacedDev{};
    const uint64_t n = r->n;
    PA_TRY(index_prepare_coverage(idx, st));
    if (n == 0) return PA_OK;
    int64_t *d_ws = nullptr;
    unsigned long long *d_err = nullptr;
    // classification, list offsets and lists: the assign pass, left on the device
    PA_TRY(assign_pass_device(idx, r, p, list_cap, out.as, b, st));
    const uint64_t total = out.as.total;
    if (total == 0 || !out.as.lists) return PA_OK;  // (nothing listed, or the capacity is short: nothing to place)
    PA_HIP(b.get(&d_err, 16));
    PA_HIP(hipMemsetAsync(d_err, 0, 16, st));
    if (want_starts) PA_HIP(b.get(&out.starts, total * 8));
    if (want_agree) PA_HIP(b.get(&out.agree, total));
    const uint32_t wmax = r->max_len >= (uint64_t)idx->k ? (uint32_t)(r->max_len - idx->k + 1) : 1;
    const uint32_t rounds = std::max<uint32_t>(1, (wmax + 63) / 64);
    // waves to fill the device (256 CUs x 16) while the lanes' diagonals stay within 64 MiB
    uint64_t blocks = std::min<uint64_t>((total + 3) / 4, 1024);
    while (blocks > 1 && blocks * 4 * rounds * 64 * 8 > (64ull << 20)) blocks /= 2;
    PA_HIP(b.get(&d_ws, blocks * 4 * rounds * 64 * 8));
    PlaceArgs a{};
    a.table = idx->table;
    a.cap = idx->cap;
    a.home = idx->home;
    a.G = idx->n_genomes;
    a.k = (int)idx->k;
    a.class_genomes = idx->class_genomes;
    a.class_mask = idx->n_genomes <= 64 ? idx->class_mask : nullptr;
    a.goff = idx->goff;
    a.head = idx->cov_head;
    a.first = idx->cov_first;
    a.n_pairs = idx->cov_pairs;
    a.seq = r->seq;
    a.off = r->off;
    a.n_reads = n;
    a.type = out.as.type;
    a.list_off = out.as.off;
    a.lists = out.as.lists;
    a.n_entries = total;
    a.starts = out.starts;
    a.agree = out.agree;
    a.diff = acc ? acc->diff : nullptr;
    a.entries = acc ? acc->entries : 0;
    a.foff = acc ? acc->foff : nullptr;
    a.both = idx->both_strands;
    a.ws = d_ws;
    a.rounds = rounds;
    a.err = d_err;
    with_nw(idx->nw, [&](auto w) { launch_place<w()>(a, (unsigned)blocks, st); });
    PA_HIP(hipGetLastError());
    if (acc) acc->depth_valid = 0;
    unsigned long long errs[2] = {0, 0};
    PA_HIP(hipMemcpyAsync(errs, d_err, 16, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    b.free(d_ws);  // (up to 64 MiB: not held through the caller's copies)
    if (errs[0] || errs[1]) {
        set_error(std::string(err_op()) + ": " + std::to_string(errs[0]) + " listed genomes without a voting window, " +
                  std::to_string(errs[1]) + " positions-view entries out of range (invariant violated)");
        return PA_EINTERNAL;
    }
    out.placed = true;
    return PA_OK;
}

pa_status coverage_place(pa_index *idx, const pa_reads *r, const DevParams &p, pa_coverage *acc, uint8_t *type,
                         uint64_t *list_off, uint32_t *lists, int64_t *starts, uint64_t list_cap,
                         uint64_t *list_total, hipStream_t st) {
    const char *what = acc ? "pa_coverage_add" : "pa_align_placements";
    const uint64_t n = r->n;
    if (list_off) list_off[0] = 0;
    if (list_total) *list_total = 0;
    const bool want_lists = lists || starts;
    ErrOp op(what);
    Bufs b(st);
    PlacedDev pd;
    // (no lists for the *list_total query, or when the caller's capacity is short)
    PA_TRY(place_device(idx, r, p, acc, acc ? ~0ull : (want_lists ? list_cap : 0), starts != nullptr, false, pd,
                        b, st));
    if (n == 0) return PA_OK;
    const uint64_t total = pd.as.total;
    if (acc) acc->reads_added += n;
    if (type) PA_HIP(hipMemcpyAsync(type, pd.as.type, n, hipMemcpyDeviceToHost, st));
    if (list_off) PA_HIP(hipMemcpyAsync(list_off, pd.as.off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (list_total) *list_total = total;
    if (want_lists && list_cap < total) {
        set_error(std::string(what) + ": list_cap smaller than the required list length");
        return PA_EINVAL;
    }
    if (pd.placed) {
        if (lists) PA_HIP(hipMemcpyAsync(lists, pd.as.lists, total * 4, hipMemcpyDeviceToHost, st));
        if (starts) PA_HIP(hipMemcpyAsync(starts, pd.starts, total * 8, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
    }
    return PA_OK;
}

// The scanned accumulator (kept until the next add or reset).
static pa_status coverage_scan(pa_coverage *cov, hipStream_t st) {
    ErrOp op("pa_coverage");
    if (cov->depth_valid) return PA_OK;
    const uint64_t n = 2 * cov->entries;
    Bufs b(st);
    if (!cov->depth) PA_HIP(pa::dev_malloc(&cov->depth, std::max<uint64_t>(n, 1) * 4));  // (the accumulator's: kept)
    if (n)
        PA_HIP(with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
            return rocprim::inclusive_scan(tmp, tmp_bytes, cov->diff, cov->depth, (size_t)n, rocprim::plus<uint32_t>(),
                                           st);
        }));
    cov->depth_valid = 1;
    return PA_OK;
}

pa_status coverage_summary(pa_coverage *cov, uint32_t min_coverage, uint64_t *cov_u, uint64_t *cov_a, uint64_t *sum_u,
                           uint64_t *sum_a, hipStream_t st) {
    ErrOp op("pa_coverage_summary");
    const uint32_t G = cov->n_genomes;
    if (G == 0) return PA_OK;
    PA_TRY(coverage_scan(cov, st));
    Bufs b(st);
    unsigned long long *d_out = nullptr;
    PA_HIP(b.get(&d_out, (uint64_t)4 * G * 8));
    hipLaunchKernelGGL(k_cover_summary, dim3(2 * G), dim3(kBlock), 0, st, cov->depth, cov->entries, cov->foff, G,
                       min_coverage, d_out);
    PA_HIP(hipGetLastError());
    std::vector<unsigned long long> h((size_t)4 * G);
    PA_HIP(hipMemcpyAsync(h.data(), d_out, (uint64_t)4 * G * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    uint64_t *outs[4] = {cov_u, cov_a, sum_u, sum_a};
    for (int i = 0; i < 4; i++)
        if (outs[i])
            for (uint32_t g = 0; g < G; g++) outs[i][g] = h[(size_t)i * G + g];
    return PA_OK;
}

pa_status coverage_depth(pa_coverage *cov, uint32_t genome, uint64_t first, uint64_t count, uint32_t *du,
                         uint32_t *da, hipStream_t st) {
    if (count == 0) return PA_OK;
    PA_TRY(coverage_scan(cov, st));
    const uint64_t at = cov->h_foff[genome] + genome + first;
    if (du) PA_HIP(hipMemcpyAsync(du, cov->depth + at, count * 4, hipMemcpyDeviceToHost, st));
    if (da) PA_HIP(hipMemcpyAsync(da, cov->depth + cov->entries + at, count * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

}  // namespace pa
