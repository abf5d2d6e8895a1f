// pa_pair.hip -- paired-end reads: mate i of two batches is one fragment, and
// the pair is classified by the union of both mates' retained k-mers (DESIGN.md
// section 15).
//
//   mates     the assign pass (pa_assign.hip) over mates 1 and over mates 2:
//             per mate its type, filter counts and list, on the device.
//   combine   k_pair_combine, one thread per pair: the pairs whose result
//             follows from the two mates' results by the reference's rule alone
//             (a dropped mate; an unmapped mate; two ambiguous mates without a
//             specific k-mer) are settled, the others queued.
//   exact     k_align_pair_exact (pa_align.hip) over the queue: lengths.
//   offsets   an exclusive scan of the pairs' list lengths, on the device.
//   lists     k_pair_copy writes the settled pairs' lists (a mate's, verbatim),
//             the exact kernel's second pass the queued pairs'.
//   cover     the type array starts as kAssignUnset; a count of the pairs still
//             holding it after the last kernel must be zero (PA_EINTERNAL).
//   count     k_pair_count adds the finished pairs to a pa_result.
// PA_PAIR_COMBINE=0 queues every pair that is not dropped (A/B runs, a fallback).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <string>

#include "pa_device.h"
#include "pa_internal.h"

namespace {

constexpr int kBlock = 256;

inline unsigned grid_for(uint64_t n) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, 65536));
}

struct Widen {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

// One mate's results (the assign pass's device arrays).
struct MateDev {
    const uint8_t *type;
    const uint32_t *qf, *hr, *len, *lists;
    const uint64_t *off;
};

enum : uint8_t { kSrcNone = 0, kSrcMate1 = 1, kSrcMate2 = 2 };  // whose list a settled pair takes

// The provable rules.  combine 0: only the dropped
// pairs are settled here.  A queued pair's number is appended wave by wave.
__global__ __launch_bounds__(kBlock) void k_pair_combine(MateDev m1, MateDev m2, uint64_t n, int combine,
                                                         uint8_t *__restrict__ type, uint32_t *__restrict__ qf,
                                                         uint32_t *__restrict__ hr, uint32_t *__restrict__ len,
                                                         uint8_t *__restrict__ src, uint32_t *__restrict__ queue,
                                                         unsigned long long *__restrict__ qcount) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t rounds = (n + stride - 1) / stride;  // uniform trip count: the ballot below is wave-wide
    for (uint64_t it = 0; it < rounds; it++) {
        const uint64_t i = it * stride + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
        bool defer = false;
        if (i < n) {
            const uint8_t t1 = m1.type[i], t2 = m2.type[i];
            uint8_t t = pa::kAssignUnset, s = kSrcNone;
            uint32_t l = 0;
            if (t1 == PA_DROPPED || t2 == PA_DROPPED) {
                t = PA_DROPPED;
            } else if (combine && t1 == PA_UNMAPPED && t2 == PA_UNMAPPED) {
                t = PA_UNMAPPED;
            } else if (combine && t2 == PA_UNMAPPED) {
                t = t1, l = m1.len[i], s = kSrcMate1;
            } else if (combine && t1 == PA_UNMAPPED) {
                t = t2, l = m2.len[i], s = kSrcMate2;
            } else if (combine && t1 == PA_AMBIGUOUSLY_MAPPED && t2 == PA_AMBIGUOUSLY_MAPPED && m1.len[i] == 0 &&
                       m2.len[i] == 0) {
                t = PA_AMBIGUOUSLY_MAPPED;
            } else {
                defer = true;
            }
            if (!defer) {
                const bool dropped = t == PA_DROPPED;
                type[i] = t;
                qf[i] = dropped ? 0 : m1.qf[i] + m2.qf[i];
                hr[i] = dropped ? 0 : m1.hr[i] + m2.hr[i];
                len[i] = l;
                src[i] = l ? s : (uint8_t)kSrcNone;
            } else {
                src[i] = kSrcNone;
            }
        }
        const uint64_t mask = __ballot(defer);
        if (mask) {
            const uint32_t lane = threadIdx.x & 63;
            unsigned long long at = 0;
            if (lane == (uint32_t)__builtin_ctzll(mask)) at = atomicAdd(qcount, (unsigned long long)__builtin_popcountll(mask));
            at = __shfl(at, __builtin_ctzll(mask));
            if (defer) queue[at + __builtin_popcountll(mask & ((1ull << lane) - 1))] = (uint32_t)i;
        }
    }
}

// The settled pairs' lists: the one mapped mate's, entry by entry.
__global__ __launch_bounds__(kBlock) void k_pair_copy(MateDev m1, MateDev m2, const uint8_t *__restrict__ src,
                                                      const uint64_t *__restrict__ off, uint64_t n, uint64_t total,
                                                      uint32_t *__restrict__ lists) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint8_t s = src[i];
        if (s == kSrcNone) continue;
        const MateDev &m = s == kSrcMate1 ? m1 : m2;
        const uint64_t from = m.off[i], o = off[i], cnt = off[i + 1] - o;
        for (uint64_t j = 0; j < cnt && o + j < total; j++) lists[o + j] = m.lists[from + j];
    }
}

// Pairs no kernel settled: one atomic per block.
__global__ __launch_bounds__(kBlock) void k_pair_unset(const uint8_t *__restrict__ type, uint64_t n,
                                                       unsigned long long *count) {
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
        c += type[i] == pa::kAssignUnset;
    __shared__ uint32_t red[kBlock / 64];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int i = 0; i < kBlock / 64; i++) s += red[i];
        if (s) atomicAdd(count, (unsigned long long)s);
    }
}

// The finished pairs into a result: the six statistics by block-level partial
// sums (one atomic per block and counter), unique / ambiguous per list entry,
// first_key = (pair index << 20) | list position by atomicMin.
__global__ __launch_bounds__(kBlock) void k_pair_count(const uint8_t *__restrict__ type, const uint32_t *__restrict__ qf,
                                                       const uint32_t *__restrict__ hr, const uint64_t *__restrict__ off,
                                                       const uint32_t *__restrict__ lists, uint64_t n, uint64_t base,
                                                       uint32_t G, unsigned long long *__restrict__ stats,
                                                       unsigned long long *__restrict__ first) {
    unsigned long long *uniq = stats + 6, *amb = uniq + G;
    unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint8_t t = type[i];
        if (t == PA_DROPPED) {
            c[3]++;
            continue;
        }
        c[t == PA_UNMAPPED ? 2 : (t == PA_UNIQUELY_MAPPED ? 0 : 1)]++;
        c[4] += qf[i];
        c[5] += hr[i];
        const uint64_t o = off[i], cnt = off[i + 1] - o;
        unsigned long long *per = t == PA_UNIQUELY_MAPPED ? uniq : amb;
        for (uint64_t j = 0; j < cnt; j++) {
            const uint32_t g = lists[o + j];
            if (g >= G) continue;  // (never: the lists hold genomes)
            atomicAdd(&per[g], 1ull);
            atomicMin(&first[g], (unsigned long long)(((base + i) << 20) | j));
        }
    }
    __shared__ unsigned long long red[6][kBlock / 64];
#pragma unroll
    for (int s = 0; s < 6; s++) {
        unsigned long long v = c[s];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if ((threadIdx.x & 63) == 0) red[s][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long v = 0;
        for (int w = 0; w < kBlock / 64; w++) v += red[threadIdx.x][w];
        if (v) atomicAdd(&stats[threadIdx.x], v);
    }
}

inline uint64_t up16(uint64_t b) { return (b + 15) / 16 * 16; }

}  // namespace

namespace pa {

pa_status align_pairs(pa_index *idx, const pa_reads *r1, const pa_reads *r2, const DevParams &p, uint64_t base,
                      pa_result *acc, uint8_t *type, uint32_t *qf, uint32_t *hr, uint64_t *list_off, uint32_t *lists,
                      uint64_t list_cap, uint64_t *list_total, uint64_t *exact_pairs, hipStream_t st) {
    const uint64_t n = r1->n;
    if (list_off) list_off[0] = 0;
    if (list_total) *list_total = 0;
    if (exact_pairs) *exact_pairs = 0;
    if (n == 0) return PA_OK;
    if (n >= 0xFFFFFFFFull) {
        set_error("pa_align_pairs: a batch holds at most 2^32 - 2 pairs (split it; pair_index_base keeps the order)");
        return PA_EUNSUPPORTED;
    }
    const bool want_lists = lists != nullptr;
    if (!want_lists) list_cap = 0;
    Bufs b(st);
    // ---- the mates' pass, lists included (a settled pair takes a mate's list)
    AssignDev d1, d2;
    PA_TRY(assign_pass_device(idx, r1, p, ~0ull, d1, b, st));
    PA_TRY(assign_pass_device(idx, r2, p, ~0ull, d2, b, st));
    const MateDev m1{d1.type, d1.qf, d1.hr, d1.len, d1.lists, d1.off};
    const MateDev m2{d2.type, d2.qf, d2.hr, d2.len, d2.lists, d2.off};
    // one allocation: off [n + 1] | qf [n] | hr [n] | len [n + 1] | queue [n] | type [n] | src [n] | counts [2]
    const uint64_t b_off = 0, b_qf = b_off + up16((n + 1) * 8), b_hr = b_qf + up16(n * 4), b_len = b_hr + up16(n * 4),
                   b_q = b_len + up16((n + 1) * 4), b_type = b_q + up16(n * 4), b_src = b_type + up16(n),
                   b_cnt = b_src + up16(n), bytes = b_cnt + 16;
    unsigned char *blk = nullptr;
    PA_HIP(b.get(&blk, bytes));
    uint64_t *d_off = (uint64_t *)(blk + b_off);
    uint32_t *d_qf = (uint32_t *)(blk + b_qf), *d_hr = (uint32_t *)(blk + b_hr), *d_len = (uint32_t *)(blk + b_len);
    uint32_t *d_queue = (uint32_t *)(blk + b_q);
    uint8_t *d_type = blk + b_type, *d_src = blk + b_src;
    unsigned long long *d_cnt = (unsigned long long *)(blk + b_cnt);  // [0] queued pairs, [1] pairs left unset
    PA_HIP(hipMemsetAsync(d_type, 0xFF, n, st));
    PA_HIP(hipMemsetAsync(d_cnt, 0, 16, st));
    PA_HIP(hipMemsetAsync(d_len + n, 0, 4, st));
    // ---- combine
    const int combine = !pa::env_is("PA_PAIR_COMBINE", '0');
    hipLaunchKernelGGL(k_pair_combine, dim3(std::min(grid_for(n), 2048u)), dim3(kBlock), 0, st, m1, m2, n, combine,
                       d_type, d_qf, d_hr, d_len, d_src, d_queue, d_cnt);
    PA_HIP(hipGetLastError());
    unsigned long long queued = 0;
    PA_HIP(hipMemcpyAsync(&queued, d_cnt, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    // ---- the queued pairs' types, counts and list lengths
    PA_TRY(pair_exact_pass(idx, r1, r2, p, d_queue, d_cnt, queued, d_type, d_qf, d_hr, d_len, nullptr, nullptr, st));
    // ---- offsets
    auto len64 = rocprim::make_transform_iterator(d_len, Widen{});
    PA_HIP(with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, len64, d_off, (uint64_t)0, (size_t)(n + 1),
                                       rocprim::plus<uint64_t>(), st);
    }));
    uint64_t total = 0;
    PA_HIP(hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    // ---- lists (always made on the device: the counters are per list entry)
    uint32_t *d_lists = nullptr;
    const bool fits = !want_lists || total <= list_cap;
    if (total > 0 && fits && (want_lists || acc)) {
        PA_HIP(b.get(&d_lists, total * 4));
        hipLaunchKernelGGL(k_pair_copy, dim3(grid_for(n)), dim3(kBlock), 0, st, m1, m2, d_src, d_off, n, total, d_lists);
        PA_HIP(hipGetLastError());
        PA_TRY(pair_exact_pass(idx, r1, r2, p, d_queue, d_cnt, queued, d_type, d_qf, d_hr, d_len, d_off, d_lists, st));
    }
    // ---- every pair settled by exactly one kernel -- at least by one: none still unset
    hipLaunchKernelGGL(k_pair_unset, dim3(std::min(grid_for(n), 2048u)), dim3(kBlock), 0, st, d_type, n, d_cnt + 1);
    PA_HIP(hipGetLastError());
    unsigned long long unset = 0;
    PA_HIP(hipMemcpyAsync(&unset, d_cnt + 1, 8, hipMemcpyDeviceToHost, st));
    if (type) PA_HIP(hipMemcpyAsync(type, d_type, n, hipMemcpyDeviceToHost, st));
    if (qf) PA_HIP(hipMemcpyAsync(qf, d_qf, n * 4, hipMemcpyDeviceToHost, st));
    if (hr) PA_HIP(hipMemcpyAsync(hr, d_hr, n * 4, hipMemcpyDeviceToHost, st));
    if (list_off) PA_HIP(hipMemcpyAsync(list_off, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (want_lists && d_lists) PA_HIP(hipMemcpyAsync(lists, d_lists, total * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (unset) {
        set_error("pa_align_pairs: " + std::to_string(unset) + " pairs were settled by no kernel (invariant violated)");
        return PA_EINTERNAL;
    }
    if (list_total) *list_total = total;
    if (exact_pairs) *exact_pairs = queued;
    if (!fits) {
        set_error("pa_align_pairs: list_cap smaller than the required list length");
        return PA_EINVAL;
    }
    // ---- counters, only now that nothing can fail any more but the device
    if (acc) {
        hipLaunchKernelGGL(k_pair_count, dim3(std::min(grid_for(n), 2048u)), dim3(kBlock), 0, st, d_type, d_qf, d_hr,
                           d_off, d_lists, n, base, idx->n_genomes, (unsigned long long *)acc->sum_block,
                           (unsigned long long *)acc->min_block);
        PA_HIP(hipGetLastError());
        PA_HIP(hipStreamSynchronize(st));
    }
    return PA_OK;
}

}  // namespace pa
