// pa_pileup.hip -- per-base pileup and SNV calls from the uniquely mapped reads:
// what the placed reads say at each genome position.  The reference has no such
// code; DESIGN.md section 13 holds the definition.
//
// Three pieces:
//
//   placement      pa_cover.hip's place_device: the assign pass left on the
//                  device, then k_place, which gives every list entry its
//                  diagonal s(read, g) and whether all voting windows agreed on it.
//   k_pileup       one wave64 per uniquely mapped read whose windows agreed:
//                  lanes take the bases i = lane, lane + 64, ..., lay them along
//                  the diagonal and add one to count[g][x][b] -- one 32-bit
//                  integer atomic per counted base, its result unused.
//   k_pileup_call  one thread per forward position: 16 B of counts, one
//                  reference code, the calling rule; run twice -- per-block
//                  record counts, a scan of them, then the records written at
//                  their ranks -- so the order (genome, position, alternative
//                  base) never depends on the schedule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <rocprim/device/device_scan.hpp>
#include <string>
#include <vector>

#include "pa_device.h"
#include "pa_internal.h"

using namespace pad;

namespace {

constexpr int kBlock = 256;
constexpr int kTiles = 16;  // k_pileup_call: tiles of kBlock positions per block

struct PileArgs {
    const uint8_t *seq, *qual;
    const uint64_t *off;
    uint64_t n_reads;
    const uint8_t *type;
    const uint64_t *list_off;
    const uint32_t *lists;
    uint64_t n_entries;
    const int64_t *starts;
    const uint8_t *agree;
    const uint64_t *goff;      // the regions
    const uint64_t *foff;      // forward bases before genome g
    uint32_t G;
    int both;
    uint32_t min_base_quality;
    uint32_t *counts;          // [4 foff[G]]
    unsigned long long *stats; // [3] reads piled, reads skipped, bases counted
};

__global__ __launch_bounds__(kBlock) void k_pileup(PileArgs a) {
    const int lane = lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    uint64_t piled = 0, skipped = 0, counted = 0;  // piled, skipped: wave-uniform; counted: this lane's
    for (uint64_t r = wave; r < a.n_reads; r += n_waves) {
        if (a.type[r] != PA_UNIQUELY_MAPPED) continue;
        const uint64_t e = a.list_off[r];  // (a unique read's list is exactly [g])
        if (e >= a.n_entries) continue;
        const uint32_t g = a.lists[e];
        if (g >= a.G) continue;  // (never: the lists hold genome numbers)
        if (!a.agree[e]) {       // its windows name two or more diagonals
            skipped++;
            continue;
        }
        piled++;
        const int64_t s = a.starts[e];
        const uint64_t off = a.off[r];
        const uint32_t len = (uint32_t)(a.off[r + 1] - off);
        const int64_t rlen = (int64_t)(a.goff[g + 1] - a.goff[g]);
        const int64_t fl = (int64_t)(a.foff[g + 1] - a.foff[g]);
        uint32_t *cg = a.counts + 4 * a.foff[g];
        for (uint32_t i = lane; i < len; i += 64) {
            const int64_t q = s + (int64_t)i;
            if (q < 0 || q >= rlen) continue;
            uint32_t b = base_code(a.seq[off + i]);
            if (b > 3) continue;
            if (a.min_base_quality && (uint32_t)a.qual[off + i] < a.min_base_quality) continue;
            int64_t x = q;
            if (a.both) {
                // region = g + N + reverse complement: q < |g| is x = q, q > |g| is x = 2|g| - q
                if (q == fl) continue;
                if (q > fl) {
                    x = 2 * fl - q;
                    b = 3 - b;
                }
            }
            atomicAdd(&cg[4 * x + b], 1u);
            counted++;
        }
    }
    counted = wave_sum64(counted);
    if (lane == 0) {
        if (piled) atomicAdd(&a.stats[0], (unsigned long long)piled);
        if (skipped) atomicAdd(&a.stats[1], (unsigned long long)skipped);
        if (counted) atomicAdd(&a.stats[2], (unsigned long long)counted);
    }
}

// The genome holding forward position t (t < foff[G]).
__device__ __forceinline__ uint32_t genome_of(const uint64_t *__restrict__ foff, uint32_t G, uint64_t t) {
    uint32_t lo = 0, hi = G;  // foff[lo] <= t < foff[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (foff[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// WRITE = false: block_n[block] = the block's records.  WRITE = true: block_n
// holds the exclusive scan of those, and the records go to out at their ranks.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void k_pileup_call(const uint4 *__restrict__ counts,
                                                        const uint8_t *__restrict__ ref,
                                                        const uint64_t *__restrict__ foff, uint32_t G, uint64_t F,
                                                        uint32_t min_depth, uint32_t min_alt_count,
                                                        uint32_t min_alt_permille, unsigned long long *block_n,
                                                        pa_variant *out, uint64_t n_out) {
    __shared__ uint32_t wsum[kBlock / 64];
    const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
    uint64_t run = WRITE ? block_n[blockIdx.x] : 0;
    uint32_t mine = 0;
    const uint64_t base = (uint64_t)blockIdx.x * kTiles * kBlock;
    for (int tile = 0; tile < kTiles; tile++) {
        const uint64_t t = base + (uint64_t)tile * kBlock + threadIdx.x;
        uint32_t mask = 0, rf = 4;
        uint4 c = make_uint4(0, 0, 0, 0);
        uint64_t D = 0;
        if (t < F) {
            c = counts[t];
            rf = ref[t];
            D = (uint64_t)c.x + c.y + c.z + c.w;
            if (rf < 4 && D >= min_depth) {
                const uint32_t cb[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (uint32_t b = 0; b < 4; b++)
                    if (b != rf && cb[b] >= min_alt_count && 1000ull * cb[b] >= (uint64_t)min_alt_permille * D)
                        mask |= 1u << b;
            }
        }
        const uint32_t cnt = (uint32_t)__popc(mask);
        if constexpr (!WRITE) {
            mine += cnt;
        } else {
            const uint32_t incl = wave_incl_scan(cnt);
            if (lane == 63) wsum[wv] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (int i = 0; i < kBlock / 64; i++) {
                before += i < wv ? wsum[i] : 0;
                total += wsum[i];
            }
            if (cnt) {
                uint64_t pos = run + before + incl - cnt;
                const uint32_t g = genome_of(foff, G, t);
                const uint32_t cb[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (uint32_t b = 0; b < 4; b++) {
                    if (!((mask >> b) & 1u)) continue;
                    if (pos < n_out) {  // (always: the count pass sized out)
                        pa_variant v;
                        v.genome = g;
                        v.ref = (uint8_t)rf;
                        v.alt = (uint8_t)b;
                        v.pad[0] = v.pad[1] = 0;
                        v.position = t - foff[g];
                        v.depth = (uint32_t)D;
                        v.alt_count = cb[b];
                        v.acgt[0] = c.x; v.acgt[1] = c.y; v.acgt[2] = c.z; v.acgt[3] = c.w;
                        out[pos] = v;
                    }
                    pos++;
                }
            }
            run += total;
            __syncthreads();
        }
    }
    if constexpr (!WRITE) {
        const uint32_t w = wave_sum(mine);
        if (lane == 0) wsum[wv] = w;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int i = 0; i < kBlock / 64; i++) s += wsum[i];
            block_n[blockIdx.x] = s;
        }
    }
}

}  // namespace

namespace pa {

pa_status pileup_create(const pa_index *idx, pa_pileup **out) {
    ErrOp op("pa_pileup_create");
    const uint32_t G = idx->n_genomes;
    const uint64_t total = idx->h_goff.empty() ? 0 : idx->h_goff[G];
    if (total >= 0xFFFFFFFFull) {
        set_error("a pileup needs a reference of fewer than 2^32 region positions (a both-strand index holds "
                  "2 |g| + 1 per genome)");
        return PA_EUNSUPPORTED;
    }
    std::unique_ptr<pa_pileup, void (*)(pa_pileup *)> p(new (std::nothrow) pa_pileup(), pileup_free);
    if (!p) {
        set_error("out of host memory");
        return PA_ENOMEM;
    }
    acc_bind(*p, idx);
    p->both = idx->both_strands;
    p->h_foff = forward_offsets(idx);
    const uint64_t F = p->h_foff[G];
    PA_HIP(pa::dev_malloc(&p->foff, (uint64_t)(G + 1) * 8));
    PA_HIP(pa::dev_malloc(&p->counts, std::max<uint64_t>(F, 1) * 16));
    PA_HIP(pa::dev_malloc(&p->ref, std::max<uint64_t>(F, 1)));
    PA_HIP(pa::dev_malloc(&p->stats, 3 * 8));
    PA_HIP(hipMemcpy(p->foff, p->h_foff.data(), (uint64_t)(G + 1) * 8, hipMemcpyHostToDevice));
    PA_HIP(hipMemset(p->counts, 0, std::max<uint64_t>(F, 1) * 16));
    PA_HIP(hipMemset(p->stats, 0, 3 * 8));
    // the forward text's codes: the first |g| codes of every region
    for (uint32_t g = 0; g < G; g++) {
        const uint64_t n = p->h_foff[g + 1] - p->h_foff[g];
        if (n) PA_HIP(hipMemcpy(p->ref + p->h_foff[g], idx->codes + idx->h_goff[g], n, hipMemcpyDeviceToDevice));
    }
    // (device memsets and copies return before they are done, and the first add may
    // come on a stream that does not wait for the null stream: all there on return)
    PA_HIP(hipStreamSynchronize(nullptr));
    *out = p.release();
    return PA_OK;
}

void pileup_free(pa_pileup *p) {
    if (!p) return;
    pa::dev_free(p->foff);
    pa::dev_free(p->counts);
    pa::dev_free(p->ref);
    pa::dev_free(p->stats);
    delete p;
}

pa_status pileup_reset(pa_pileup *p, hipStream_t st) {
    PA_HIP(hipMemsetAsync(p->counts, 0, std::max<uint64_t>(p->h_foff[p->n_genomes], 1) * 16, st));
    PA_HIP(hipMemsetAsync(p->stats, 0, 3 * 8, st));
    p->reads_added = 0;
    return PA_OK;
}

pa_status pileup_add(pa_index *idx, const pa_reads *r, const DevParams &prm, uint32_t min_base_quality, pa_pileup *acc,
                     hipStream_t st) {
    ErrOp op("pa_pileup_add");
    Bufs b(st);
    PlacedDev pd;
    PA_TRY(place_device(idx, r, prm, nullptr, ~0ull, true, true, pd, b, st));
    const uint64_t n = r->n;
    if (n == 0) return PA_OK;
    if (pd.placed) {
        PileArgs a{};
        a.seq = r->seq;
        a.qual = r->qual;
        a.off = r->off;
        a.n_reads = n;
        a.type = pd.as.type;
        a.list_off = pd.as.off;
        a.lists = pd.as.lists;
        a.n_entries = pd.as.total;
        a.starts = pd.starts;
        a.agree = pd.agree;
        a.goff = idx->goff;
        a.foff = acc->foff;
        a.G = idx->n_genomes;
        a.both = idx->both_strands;
        // (a threshold no base of the batch can fail is not applied: the qualities are then not loaded)
        a.min_base_quality = r->q_min >= 0 && (uint32_t)r->q_min >= min_base_quality ? 0 : min_base_quality;
        a.counts = acc->counts;
        a.stats = acc->stats;
        // a wave per read, the waves striding over the batch: one stats update per wave
        const unsigned blocks = (unsigned)std::min<uint64_t>((n + 3) / 4, 8192);
        hipLaunchKernelGGL(k_pileup, dim3(blocks), dim3(kBlock), 0, st, a);
        PA_HIP(hipGetLastError());
        PA_HIP(hipStreamSynchronize(st));
    }
    acc->reads_added += n;
    return PA_OK;
}

pa_status pileup_stats(const pa_pileup *p, pa_pileup_stats *out, hipStream_t st) {
    unsigned long long h[3] = {0, 0, 0};
    PA_HIP(hipMemcpyAsync(h, p->stats, sizeof h, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    out->reads_piled = h[0];
    out->reads_skipped = h[1];
    out->bases_counted = h[2];
    return PA_OK;
}

pa_status pileup_counts(const pa_pileup *p, uint32_t genome, uint64_t first, uint64_t count, uint32_t *acgt,
                        hipStream_t st) {
    if (count == 0) return PA_OK;
    PA_HIP(hipMemcpyAsync(acgt, p->counts + 4 * (p->h_foff[genome] + first), count * 16, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

pa_status pileup_variants(const pa_pileup *p, uint32_t min_depth, uint32_t min_alt_count, uint32_t min_alt_permille,
                          pa_variant *out, uint64_t cap, uint64_t *n, hipStream_t st) {
    ErrOp op("pa_pileup_variants");
    static_assert(sizeof(pa_variant) == 40, "pa_variant is 40 bytes");
    *n = 0;
    const uint64_t F = p->h_foff[p->n_genomes];
    if (F == 0) return PA_OK;
    const unsigned grid = (unsigned)((F + (uint64_t)kTiles * kBlock - 1) / ((uint64_t)kTiles * kBlock));
    unsigned long long *d_n = nullptr, *d_off = nullptr;
    pa_variant *d_out = nullptr;
    Bufs b(st);
    PA_HIP(b.get(&d_n, ((uint64_t)grid + 1) * 8));
    PA_HIP(b.get(&d_off, ((uint64_t)grid + 1) * 8));
    PA_HIP(hipMemsetAsync(d_n + grid, 0, 8, st));
    const uint4 *counts = (const uint4 *)p->counts;
    hipLaunchKernelGGL(k_pileup_call<false>, dim3(grid), dim3(kBlock), 0, st, counts, p->ref, p->foff, p->n_genomes, F,
                       min_depth, min_alt_count, min_alt_permille, d_n, (pa_variant *)nullptr, (uint64_t)0);
    PA_HIP(hipGetLastError());
    PA_HIP(with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, d_n, d_off, 0ull, (size_t)grid + 1,
                                       rocprim::plus<unsigned long long>(), st);
    }));
    unsigned long long total = 0;
    PA_HIP(hipMemcpyAsync(&total, d_off + grid, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    *n = total;
    if (total > cap) {
        set_error("pa_pileup_variants: cap smaller than the number of records");
        return PA_EINVAL;
    }
    if (total == 0) return PA_OK;
    PA_HIP(b.get(&d_out, total * sizeof(pa_variant)));
    hipLaunchKernelGGL(k_pileup_call<true>, dim3(grid), dim3(kBlock), 0, st, counts, p->ref, p->foff, p->n_genomes, F,
                       min_depth, min_alt_count, min_alt_permille, d_off, d_out, (uint64_t)total);
    PA_HIP(hipGetLastError());
    PA_HIP(hipMemcpyAsync(out, d_out, total * sizeof(pa_variant), hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

}  // namespace pa
