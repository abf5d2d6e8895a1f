// pa_abund.hip -- genome abundance: the reads' compatibility classes and an EM
// over them.  DESIGN.md section 14.
//
//   types      the assign pass (pa_assign.hip) leaves every read's type and the
//              unique reads' genome on the device; k_abund_types counts the
//              types, counts the unique reads per genome (they never reach the
//              sort) and queues the ambiguous reads.
//   sets       k_abund_cand (pa_align.hip, k_align_exact's front half) walks
//              the queued reads only: set sizes, a scan, the sets.
//   interning  a 64-bit hash of every queued read's set, a radix sort of
//              (hash, read), run heads, and k_abund_verify compares every
//              read's set with its run head's: a difference under an equal
//              hash is never merged -- the batch is hashed again with another
//              seed, three times at most.  The batch's classes (a few thousand)
//              go to the host, which merges them into the accumulator.
//   EM         E-step over the classes, M-step as a gather over the genome ->
//              class transpose (classes ascending), a one-block max reduction
//              for the delta: double precision, no floating-point atomics,
//              every sum in a fixed order.
//   bootstrap   B resamples of the reads over their
//              classes, draw by draw in integers (k_boot_draw, a grid strip per
//              replicate), then the same EM on every resample, a workgroup per
//              replicate and the whole loop in one launch (k_boot_em).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <string>

#include "pa_device.h"
#include "pa_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kLdsGenomes = 2048;  // unique reads per genome counted in LDS up to this many genomes (8 KB)
constexpr int kHashTries = 3;

inline unsigned grid_for(uint64_t n, unsigned cap = 4096) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, cap));
}

struct Widen {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

// Per read of the batch: its type counted, a unique read counted for its genome
// (the one entry of its list) and given a set of one, an ambiguous read queued
// (one atomic per wave), every other read given an empty set.
// counts: [0..3] reads unique, ambiguous, unmapped, dropped; [4 + g] unique reads of g.
__global__ __launch_bounds__(kBlock) void k_abund_types(const uint8_t *__restrict__ type,
                                                        const uint64_t *__restrict__ list_off,
                                                        const uint32_t *__restrict__ lists, uint64_t n, uint32_t G,
                                                        uint32_t *__restrict__ queue, unsigned long long *qcount,
                                                        uint32_t *__restrict__ set_len, unsigned long long *counts) {
    __shared__ uint32_t hist[kLdsGenomes];
    __shared__ uint32_t tcnt[4];
    const bool lds = G <= kLdsGenomes;
    if (lds)
        for (uint32_t g = threadIdx.x; g < G; g += kBlock) hist[g] = 0;
    if (threadIdx.x < 4) tcnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mine[4] = {0, 0, 0, 0};  // unique, ambiguous, unmapped, dropped
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t t = i < n ? type[i] : 0xFFu;
        const bool amb = t == PA_AMBIGUOUSLY_MAPPED;
        const uint64_t m = __ballot(amb);
        if (m) {
            const int lane = pad::lane_id();
            unsigned long long at = 0;
            if (lane == __ffsll((long long)m) - 1) at = atomicAdd(qcount, (unsigned long long)__popcll(m));
            at = pad::shfl64(at, __ffsll((long long)m) - 1);
            if (amb) queue[at + __popcll(m & ((1ull << lane) - 1))] = (uint32_t)i;
        }
        if (i >= n) continue;
        if (t == PA_UNIQUELY_MAPPED) {
            const uint32_t g = lists[list_off[i]];
            if (g < G) {
                if (lds)
                    atomicAdd(&hist[g], 1u);
                else
                    atomicAdd(&counts[4 + g], 1ull);
            }
            set_len[i] = 1;
            mine[0]++;
        } else {
            if (!amb) set_len[i] = 0;  // (the candidate kernel writes the ambiguous reads')
            mine[amb ? 1 : t == PA_UNMAPPED ? 2 : 3]++;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t s = pad::wave_sum(mine[j]);
        if (pad::lane_id() == 0 && s) atomicAdd(&tcnt[j], s);
    }
    __syncthreads();
    if (threadIdx.x < 4 && tcnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)tcnt[threadIdx.x]);
    if (lds)
        for (uint32_t g = threadIdx.x; g < G; g += kBlock)
            if (hist[g]) atomicAdd(&counts[4 + g], (unsigned long long)hist[g]);
}

// The unique reads' sets: their one genome at their offset.
__global__ __launch_bounds__(kBlock) void k_abund_unique_sets(const uint8_t *__restrict__ type,
                                                              const uint64_t *__restrict__ list_off,
                                                              const uint32_t *__restrict__ lists,
                                                              const uint64_t *__restrict__ set_off, uint64_t n,
                                                              uint64_t total, uint32_t *__restrict__ sets) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        if (type[i] != PA_UNIQUELY_MAPPED) continue;
        const uint64_t o = set_off[i];
        if (o < total) sets[o] = lists[list_off[i]];
    }
}

// (hash of its set, read) for every queued read; err[1]: an ambiguous read with an empty set.
__global__ __launch_bounds__(kBlock) void k_abund_hash(const uint32_t *__restrict__ queue, uint64_t nq,
                                                       const uint64_t *__restrict__ set_off,
                                                       const uint32_t *__restrict__ sets, uint64_t seed,
                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                       uint32_t *err) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t r = queue[j];
        const uint64_t o = set_off[r], e = set_off[r + 1];
        if (e == o) atomicOr(&err[1], 1u);
        uint64_t h = pad::fmix64(seed ^ (e - o));
        for (uint64_t i = o; i < e; i++) h = pad::fmix64(h ^ ((uint64_t)sets[i] + 0x9E3779B97F4A7C15ull));
        keys[j] = h;
        vals[j] = r;
    }
}

// 1 at the first entry of every run of equal keys.
__global__ __launch_bounds__(kBlock) void k_abund_flags(const uint64_t *__restrict__ keys, uint64_t nq,
                                                        uint32_t *__restrict__ flag) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * kBlock)
        flag[j] = j == 0 || keys[j] != keys[j - 1];
}

// head[run] = the run's first entry (rid: the inclusive scan of the flags; run = rid - 1).
__global__ __launch_bounds__(kBlock) void k_abund_heads(const uint32_t *__restrict__ flag,
                                                        const uint32_t *__restrict__ rid, uint64_t nq,
                                                        uint32_t *__restrict__ head) {
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * kBlock)
        if (flag[j]) head[rid[j] - 1] = (uint32_t)j;
}

// Every read's set against its run head's (err[0] on a difference); the heads
// write their run's set size and read count.
__global__ __launch_bounds__(kBlock) void k_abund_verify(const uint32_t *__restrict__ vals,
                                                         const uint32_t *__restrict__ flag,
                                                         const uint32_t *__restrict__ rid,
                                                         const uint32_t *__restrict__ head, uint64_t nq,
                                                         const uint64_t *__restrict__ set_off,
                                                         const uint32_t *__restrict__ sets,
                                                         uint32_t *__restrict__ run_len,
                                                         unsigned long long *__restrict__ run_cnt, uint32_t *err) {
    const uint32_t n_runs = rid[nq - 1];
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * kBlock) {
        const uint32_t run = rid[j] - 1, hj = head[run];
        const uint32_t ra = vals[j], rb = vals[hj];
        const uint64_t oa = set_off[ra], ob = set_off[rb];
        const uint64_t la = set_off[ra + 1] - oa, lb = set_off[rb + 1] - ob;
        if (flag[j]) {
            run_len[run] = (uint32_t)la;
            run_cnt[run] = (run + 1 < n_runs ? (uint64_t)head[run + 1] : nq) - j;
        } else {
            bool same = la == lb;
            for (uint64_t i = 0; same && i < la; i++) same = sets[oa + i] == sets[ob + i];
            if (!same) atomicOr(&err[0], 1u);
        }
    }
}

// The runs' sets, one after the other (a wave per run, the lanes over its genomes).
__global__ __launch_bounds__(kBlock) void k_abund_gather(const uint32_t *__restrict__ vals,
                                                         const uint32_t *__restrict__ head, uint32_t n_runs,
                                                         const uint64_t *__restrict__ set_off,
                                                         const uint32_t *__restrict__ sets,
                                                         const uint64_t *__restrict__ run_off, uint64_t entries,
                                                         uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t run = (uint64_t)blockIdx.x * (kBlock / 64) + wave; run < n_runs;
         run += (uint64_t)gridDim.x * (kBlock / 64)) {
        const uint32_t r = vals[head[run]];
        const uint64_t o = set_off[r], len = set_off[r + 1] - o, d = run_off[run];
        for (uint64_t i = lane; i < len; i += 64)
            if (d + i < entries) out[d + i] = sets[o + i];
    }
}

// ---- the EM ------------------------------------------------------------------

// theta_g / L_g (a genome shorter than k holds no k-mer, is in no class and has none)
__host__ __device__ inline double rho_of(double theta, double len) { return len >= 1.0 ? theta / len : 0.0; }

// E-step, a thread per class: d_C = sum of theta_g / L_g over its list, in list order.
__global__ __launch_bounds__(kBlock) void k_em_e(const uint64_t *__restrict__ c_off, const uint32_t *__restrict__ c_g,
                                                 uint32_t n_classes, const double *__restrict__ theta,
                                                 const double *__restrict__ len, double *__restrict__ d) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_classes) return;
    double s = 0;
    for (uint64_t i = c_off[c]; i < c_off[c + 1]; i++) {
        const uint32_t g = c_g[i];
        s += rho_of(theta[g], len[g]);
    }
    d[c] = s;
}

// M-step, a thread per genome: the gather over its classes (ascending), then |theta' - theta|.
__global__ __launch_bounds__(kBlock) void k_em_m(const uint64_t *__restrict__ t_off, const uint32_t *__restrict__ t_c,
                                                 uint32_t G, const double *__restrict__ theta,
                                                 const double *__restrict__ len, const double *__restrict__ n_c,
                                                 const double *__restrict__ d, double n_total,
                                                 double *__restrict__ theta_new, double *__restrict__ diff) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= G) return;
    const double rho = rho_of(theta[g], len[g]);
    double s = 0;
    for (uint64_t i = t_off[g]; i < t_off[g + 1]; i++) {
        const uint32_t c = t_c[i];
        const double dc = d[c];
        if (dc != 0) s += n_c[c] * rho / dc;
    }
    const double t = s / n_total;
    theta_new[g] = t;
    diff[g] = fabs(t - theta[g]);
}

// max of diff[0 .. G) by one block: a shape that does not depend on a grid (and
// max is exact in any order).
__global__ __launch_bounds__(kBlock) void k_em_delta(const double *__restrict__ diff, uint32_t G, double *out) {
    __shared__ double red[kBlock];
    double m = 0;
    for (uint32_t g = threadIdx.x; g < G; g += kBlock) m = fmax(m, diff[g]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// ---- the bootstrap --------------------------------------

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
// cum and the block's histogram are kept in LDS up to this many classes:
// (4096 + 1) * 8 + 4096 * 4 bytes = 48 KB + 8, dynamic, sized by the classes held.
constexpr uint32_t kBootLdsClasses = 4096;
constexpr uint64_t kBootBlockDraws = 1ull << 31;  // a block's draws at most: its uint32 histogram cannot wrap

inline size_t boot_lds_bytes(uint32_t nc) { return ((size_t)nc + 1) * 8 + (size_t)nc * 4; }

// Replicate blockIdx.y, draws blockIdx.x * kBlock + threadIdx.x, + gridDim.x * kBlock, ...:
// draw i is r = floor(fmix64(key_b + golden * i) * N / 2^64), counted in the
// class c with cum[c] <= r < cum[c + 1] (cum: nc + 1 entries, strictly
// ascending, cum[nc] = N > r).  Integers only.  LDS: cum and a uint32 histogram
// in (dynamic) LDS, flushed with one 64-bit atomic per class the block touched;
// otherwise cum from global memory and a 64-bit atomic per draw.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_boot_draw(const uint64_t *__restrict__ cum, uint32_t nc, uint64_t N,
                                                      uint64_t seed, unsigned long long *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char boot_lds[];
    uint64_t *s_cum = (uint64_t *)boot_lds;
    uint32_t *s_hist = (uint32_t *)(boot_lds + ((size_t)nc + 1) * 8);
    const uint32_t b = blockIdx.y;
    unsigned long long *mine = counts + (uint64_t)b * nc;
    if (LDS) {
        for (uint32_t c = threadIdx.x; c <= nc; c += kBlock) s_cum[c] = cum[c];
        for (uint32_t c = threadIdx.x; c < nc; c += kBlock) s_hist[c] = 0;
        __syncthreads();
    }
    const uint64_t *cm = LDS ? s_cum : cum;
    const uint64_t key = pad::fmix64(seed + kGolden * ((uint64_t)b + 1));
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = __umul64hi(pad::fmix64(key + kGolden * i), N);
        uint32_t lo = 0, hi = nc;  // cm[lo] <= r < cm[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (cm[mid] <= r)
                lo = mid;
            else
                hi = mid;
        }
        if (LDS)
            atomicAdd(&s_hist[lo], 1u);
        else
            atomicAdd(&mine[lo], 1ull);
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < nc; c += kBlock)
            if (s_hist[c]) atomicAdd(&mine[c], (unsigned long long)s_hist[c]);
    }
}

// The EM of replicate blockIdx.x, the whole loop in one launch: k_em_e's and
// k_em_m's sums term for term with the replicate's counts for n_C, the classes
// and then the genomes strided over the workgroup's threads.  d and the two
// thetas are the replicate's rows of global scratch: what one phase writes the
// next reads from other threads of the workgroup, through agent-scope accesses
// with a barrier between the phases; LDS holds the max reduction only.
__global__ __launch_bounds__(kBlock) void k_boot_em(const uint64_t *__restrict__ c_off, const uint32_t *__restrict__ c_g,
                                                    const uint64_t *__restrict__ t_off, const uint32_t *__restrict__ t_c,
                                                    uint32_t nc, uint32_t G, const double *__restrict__ len,
                                                    const unsigned long long *__restrict__ counts, double n_total,
                                                    uint32_t max_iterations, double tolerance, double *d_all,
                                                    double *theta_all, double *__restrict__ theta_out,
                                                    uint32_t *__restrict__ iterations, double *__restrict__ delta_out) {
    __shared__ double red[kBlock];
    const uint32_t b = blockIdx.x;
    const unsigned long long *n_c = counts + (uint64_t)b * nc;
    double *d = d_all + (uint64_t)b * nc;
    double *theta = theta_all + (uint64_t)b * 2 * G, *theta_new = theta + G;
    for (uint32_t g = threadIdx.x; g < G; g += kBlock) pad::st_agent(&theta[g], 1.0 / (double)G);
    __syncthreads();
    uint32_t it = 0;
    double delta = 0;
    while (it < max_iterations) {
        for (uint32_t c = threadIdx.x; c < nc; c += kBlock) {
            double s = 0;
            for (uint64_t i = c_off[c]; i < c_off[c + 1]; i++) {
                const uint32_t g = c_g[i];
                s += rho_of(pad::ld_agent(&theta[g]), len[g]);
            }
            pad::st_agent(&d[c], s);
        }
        __syncthreads();
        double m = 0;
        for (uint32_t g = threadIdx.x; g < G; g += kBlock) {
            const double th = pad::ld_agent(&theta[g]);
            const double rho = rho_of(th, len[g]);
            double s = 0;
            for (uint64_t i = t_off[g]; i < t_off[g + 1]; i++) {
                const uint32_t c = t_c[i];
                const double dc = pad::ld_agent(&d[c]);
                const double n = (double)n_c[c];
                if (dc != 0) s += n * rho / dc;
            }
            const double t = s / n_total;
            pad::st_agent(&theta_new[g], t);
            m = fmax(m, fabs(t - th));
        }
        red[threadIdx.x] = m;
        __syncthreads();
        for (int s = kBlock / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
            __syncthreads();
        }
        delta = red[0];
        __syncthreads();  // (red is written again in the next iteration)
        double *sw = theta;
        theta = theta_new;
        theta_new = sw;
        it++;
        if (tolerance > 0 && delta < tolerance) break;  // (uniform: every thread read the same red[0])
    }
    for (uint32_t g = threadIdx.x; g < G; g += kBlock) theta_out[(uint64_t)b * G + g] = pad::ld_agent(&theta[g]);
    if (threadIdx.x == 0) {
        iterations[b] = it;
        delta_out[b] = delta;
    }
}

using pa::Bufs;
using pa::CandDev;

}  // namespace

// The candidate pass left on the device (declared in pa_internal.h: pa_lineage.hip starts from it too).
pa_status pa::candidates_device(pa_index *idx, const pa_reads *r, const pa::DevParams &p, uint64_t cap,
                                unsigned long long *counts, CandDev &out, Bufs &b, hipStream_t st) {
    const uint64_t n = r->n;
    const uint32_t G = idx->n_genomes;
    PA_TRY(pa::assign_pass_device(idx, r, p, ~0ull, out.as, b, st));
    unsigned long long *d_qcount = nullptr;
    PA_HIP(b.get(&out.queue, n * 4));
    PA_HIP(b.get(&out.len, (n + 1) * 4));
    PA_HIP(b.get(&out.off, (n + 1) * 8));
    PA_HIP(b.get(&d_qcount, 8));
    if (!counts) {
        PA_HIP(b.get(&counts, (4 + (uint64_t)G) * 8));
        PA_HIP(hipMemsetAsync(counts, 0, (4 + (uint64_t)G) * 8, st));
    }
    PA_HIP(hipMemsetAsync(d_qcount, 0, 8, st));
    PA_HIP(hipMemsetAsync(out.len + n, 0, 4, st));
    hipLaunchKernelGGL(k_abund_types, dim3(grid_for(n, 1024)), dim3(kBlock), 0, st, out.as.type, out.as.off,
                       out.as.lists, n, G, out.queue, d_qcount, out.len, counts);
    PA_HIP(hipGetLastError());
    unsigned long long nq = 0;
    PA_HIP(hipMemcpyAsync(&nq, d_qcount, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    out.nq = nq;
    PA_TRY(pa::candidates_pass(idx, r, p, out.queue, d_qcount, nq, out.len, nullptr, nullptr, st));
    auto len64 = rocprim::make_transform_iterator(out.len, Widen{});
    PA_HIP(pa::with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, len64, out.off, (uint64_t)0, (size_t)(n + 1),
                                       rocprim::plus<uint64_t>(), st);
    }));
    uint64_t total = 0;
    PA_HIP(hipMemcpyAsync(&total, out.off + n, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    out.total = total;
    if (total == 0 || total > cap) return PA_OK;
    PA_HIP(b.get(&out.sets, total * 4));
    if (out.as.lists) {
        hipLaunchKernelGGL(k_abund_unique_sets, dim3(grid_for(n)), dim3(kBlock), 0, st, out.as.type, out.as.off,
                           out.as.lists, out.off, n, total, out.sets);
        PA_HIP(hipGetLastError());
    }
    return pa::candidates_pass(idx, r, p, out.queue, d_qcount, nq, out.len, out.off, out.sets, st);
}

namespace {

// One batch's ambiguous reads reduced to classes and merged into acc->classes.
pa_status intern_batch(const CandDev &c, pa_abundance *acc, Bufs &b, hipStream_t st) {
    const uint64_t nq = c.nq;
    if (nq == 0) return PA_OK;
    uint64_t *keys = nullptr, *keys2 = nullptr, *run_off = nullptr;
    uint32_t *vals = nullptr, *vals2 = nullptr, *flag = nullptr, *rid = nullptr, *head = nullptr, *run_len = nullptr,
             *err = nullptr;
    unsigned long long *run_cnt = nullptr;
    PA_HIP(b.get(&keys, nq * 8));
    PA_HIP(b.get(&keys2, nq * 8));
    PA_HIP(b.get(&vals, nq * 4));
    PA_HIP(b.get(&vals2, nq * 4));
    PA_HIP(b.get(&flag, nq * 4));
    PA_HIP(b.get(&rid, nq * 4));
    PA_HIP(b.get(&head, nq * 4));
    PA_HIP(b.get(&run_len, (nq + 1) * 4));
    PA_HIP(b.get(&run_cnt, nq * 8));
    PA_HIP(b.get(&run_off, (nq + 1) * 8));
    PA_HIP(b.get(&err, 8));
    size_t sort_bytes = 0, scan_bytes = 0;  // (one temporary for the sort and the scan of every attempt)
    auto len64 = rocprim::make_transform_iterator(run_len, Widen{});
    PA_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, keys2, vals, vals2, (size_t)nq, 0, 64, st));
    PA_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, flag, rid, (size_t)nq, rocprim::plus<uint32_t>(), st));
    void *tmp = nullptr;
    PA_HIP(b.get(&tmp, std::max(sort_bytes, scan_bytes)));
    const unsigned grid = grid_for(nq);
    for (int attempt = 0;; attempt++) {
        const uint64_t seed = 0x243F6A8885A308D3ull + 0x9E3779B97F4A7C15ull * (uint64_t)attempt;
        PA_HIP(hipMemsetAsync(err, 0, 8, st));
        hipLaunchKernelGGL(k_abund_hash, dim3(grid), dim3(kBlock), 0, st, c.queue, nq, c.off, c.sets, seed, keys, vals,
                           err);
        PA_HIP(hipGetLastError());
        PA_HIP(rocprim::radix_sort_pairs(tmp, sort_bytes, keys, keys2, vals, vals2, (size_t)nq, 0, 64, st));
        hipLaunchKernelGGL(k_abund_flags, dim3(grid), dim3(kBlock), 0, st, keys2, nq, flag);
        PA_HIP(hipGetLastError());
        PA_HIP(rocprim::inclusive_scan(tmp, scan_bytes, flag, rid, (size_t)nq, rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL(k_abund_heads, dim3(grid), dim3(kBlock), 0, st, flag, rid, nq, head);
        PA_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_abund_verify, dim3(grid), dim3(kBlock), 0, st, vals2, flag, rid, head, nq, c.off, c.sets,
                           run_len, run_cnt, err);
        PA_HIP(hipGetLastError());
        uint32_t h_err[2] = {0, 0};
        PA_HIP(hipMemcpyAsync(h_err, err, 8, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
        if (h_err[1]) {
            pa::set_error("pa_abundance_add: an ambiguous read has no candidate genome (invariant violated)");
            return PA_EINTERNAL;
        }
        if (!h_err[0]) break;
        if (attempt + 1 == kHashTries) {
            pa::set_error("pa_abundance_add: two different genome sets shared a hash under three seeds");
            return PA_EINTERNAL;
        }
    }
    uint32_t n_runs = 0;
    PA_HIP(hipMemcpyAsync(&n_runs, rid + (nq - 1), 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    PA_HIP(hipMemsetAsync(run_len + n_runs, 0, 4, st));
    PA_HIP(pa::with_temp(b, [&](void *tmp2, size_t &scan2_bytes) {
        return rocprim::exclusive_scan(tmp2, scan2_bytes, len64, run_off, (uint64_t)0, (size_t)n_runs + 1,
                                       rocprim::plus<uint64_t>(), st);
    }));
    uint64_t entries = 0;
    PA_HIP(hipMemcpyAsync(&entries, run_off + n_runs, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    uint32_t *run_g = nullptr;
    PA_HIP(b.get(&run_g, entries * 4));
    hipLaunchKernelGGL(k_abund_gather, dim3(grid_for((uint64_t)n_runs * 64)), dim3(kBlock), 0, st, vals2, head, n_runs,
                       c.off, c.sets, run_off, entries, run_g);
    PA_HIP(hipGetLastError());
    // per class, not per read: the batch's classes to the host and into the accumulator
    std::vector<uint64_t> h_off((size_t)n_runs + 1), h_cnt(n_runs);
    std::vector<uint32_t> h_g(entries);
    PA_HIP(hipMemcpyAsync(h_off.data(), run_off, ((size_t)n_runs + 1) * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(h_cnt.data(), run_cnt, (size_t)n_runs * 8, hipMemcpyDeviceToHost, st));
    if (entries) PA_HIP(hipMemcpyAsync(h_g.data(), run_g, entries * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n_runs; i++)
        acc->classes[std::vector<uint32_t>(h_g.begin() + h_off[i], h_g.begin() + h_off[i + 1])] += h_cnt[i];
    return PA_OK;
}

// The accumulator's classes in reported order: the ambiguous reads' classes with
// the unique reads of g added to {g}.
pa_status collect(const pa_abundance *a, hipStream_t st, std::map<std::vector<uint32_t>, uint64_t> &m,
                  uint64_t *types /* [4], nullable */) {
    const uint32_t G = a->n_genomes;
    std::vector<unsigned long long> h(4 + (size_t)G);
    PA_HIP(hipMemcpyAsync(h.data(), a->counts, h.size() * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    m = a->classes;
    for (uint32_t g = 0; g < G; g++)
        if (h[4 + g]) m[std::vector<uint32_t>{g}] += h[4 + g];
    if (types)
        for (int i = 0; i < 4; i++) types[i] = h[i];
    return PA_OK;
}

// The classes in reported order as a CSR (class -> genomes), its transpose
// (genome -> classes, ascending) and their counts: what the EM kernels read.
struct ClassTables {
    uint32_t nc = 0;
    std::vector<uint64_t> c_off, t_off, n;
    std::vector<uint32_t> c_g, t_c;
    void build(const std::map<std::vector<uint32_t>, uint64_t> &m, uint32_t G) {
        uint64_t E = 0;
        for (const auto &kv : m) E += kv.first.size();
        nc = (uint32_t)m.size();
        c_off.assign((size_t)nc + 1, 0);
        t_off.assign((size_t)G + 1, 0);
        n.resize(nc);
        c_g.resize(E);
        t_c.resize(E);
        uint32_t c = 0;
        uint64_t o = 0;
        for (const auto &kv : m) {
            n[c] = kv.second;
            for (uint32_t g : kv.first) c_g[o++] = g, t_off[g + 1]++;
            c_off[++c] = o;
        }
        for (uint32_t g = 0; g < G; g++) t_off[g + 1] += t_off[g];
        std::vector<uint64_t> at(t_off.begin(), t_off.end() - 1);
        for (c = 0; c < nc; c++)
            for (uint64_t i = c_off[c]; i < c_off[c + 1]; i++) t_c[at[c_g[i]]++] = c;
    }
};

}  // namespace

namespace pa {

pa_status abundance_create(const pa_index *idx, pa_abundance **out) {
    ErrOp op("pa_abundance_create");
    std::unique_ptr<pa_abundance, void (*)(pa_abundance *)> a(new (std::nothrow) pa_abundance(), abundance_free);
    if (!a) {
        set_error("out of host memory");
        return PA_ENOMEM;
    }
    const uint32_t G = idx->n_genomes;
    acc_bind(*a, idx);
    for (uint64_t len : forward_lengths(idx)) a->h_len.push_back((double)len - (double)idx->k + 1.0);
    PA_HIP(pa::dev_malloc(&a->counts, (4 + (uint64_t)G) * 8));
    PA_HIP(hipMemset(a->counts, 0, (4 + (uint64_t)G) * 8));
    PA_HIP(hipStreamSynchronize(nullptr));
    *out = a.release();
    return PA_OK;
}

void abundance_free(pa_abundance *a) {
    if (!a) return;
    pa::dev_free(a->counts);
    delete a;
}

pa_status abundance_reset(pa_abundance *a, hipStream_t st) {
    PA_HIP(hipMemsetAsync(a->counts, 0, (4 + (uint64_t)a->n_genomes) * 8, st));
    PA_HIP(hipStreamSynchronize(st));
    a->classes.clear();
    return PA_OK;
}

pa_status abundance_add(pa_index *idx, const pa_reads *r, const DevParams &p, pa_abundance *acc, hipStream_t st) {
    if (r->n == 0) return PA_OK;
    Bufs b(st);
    CandDev c;
    PA_TRY(candidates_device(idx, r, p, ~0ull, acc->counts, c, b, st));
    return intern_batch(c, acc, b, st);
}

pa_status align_candidates(pa_index *idx, const pa_reads *r, const DevParams &p, uint8_t *type, uint64_t *set_off,
                           uint32_t *sets, uint64_t cap, uint64_t *total, hipStream_t st) {
    const uint64_t n = r->n;
    set_off[0] = 0;
    *total = 0;
    if (n == 0) return PA_OK;
    if (!sets) cap = 0;
    Bufs b(st);
    CandDev c;
    PA_TRY(candidates_device(idx, r, p, cap, nullptr, c, b, st));
    PA_HIP(hipMemcpyAsync(type, c.as.type, n, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(set_off, c.off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (c.sets) PA_HIP(hipMemcpyAsync(sets, c.sets, c.total * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    *total = c.total;
    if (c.total > cap) {
        set_error("pa_align_candidates: cap smaller than the required length");
        return PA_EINVAL;
    }
    return PA_OK;
}

pa_status abundance_info(const pa_abundance *a, pa_abundance_info *out, hipStream_t st) {
    std::map<std::vector<uint32_t>, uint64_t> m;
    uint64_t t[4];
    PA_TRY(collect(a, st, m, t));
    out->reads_unique = t[0];
    out->reads_ambiguous = t[1];
    out->reads_unmapped = t[2];
    out->reads_dropped = t[3];
    out->n_classes = m.size();
    out->class_entries = 0;
    for (const auto &kv : m) out->class_entries += kv.first.size();
    return PA_OK;
}

pa_status abundance_classes(const pa_abundance *a, uint64_t *class_off, uint32_t *genomes, uint64_t *counts,
                            uint64_t cap_classes, uint64_t cap_entries, uint64_t *n_classes, uint64_t *n_entries,
                            hipStream_t st) {
    std::map<std::vector<uint32_t>, uint64_t> m;
    PA_TRY(collect(a, st, m, nullptr));
    uint64_t entries = 0;
    for (const auto &kv : m) entries += kv.first.size();
    *n_classes = m.size();
    *n_entries = entries;
    if (!class_off || !counts) cap_classes = 0;
    if (!genomes) cap_entries = 0;
    if (m.size() > cap_classes || entries > cap_entries) {
        set_error("pa_abundance_classes: capacity smaller than the classes held");
        return PA_EINVAL;
    }
    uint64_t c = 0, o = 0;
    for (const auto &kv : m) {
        class_off[c] = o;
        counts[c++] = kv.second;
        for (uint32_t g : kv.first) genomes[o++] = g;
    }
    if (class_off) class_off[c] = o;
    return PA_OK;
}

pa_status abundance_estimate(const pa_abundance *a, uint32_t max_iterations, double tolerance, double *read_fraction,
                             double *abundance, uint32_t *iterations_done, double *last_delta, hipStream_t st) {
    const uint32_t G = a->n_genomes;
    if (read_fraction) std::fill(read_fraction, read_fraction + G, 0.0);
    if (abundance) std::fill(abundance, abundance + G, 0.0);
    if (iterations_done) *iterations_done = 0;
    if (last_delta) *last_delta = 0;
    std::map<std::vector<uint32_t>, uint64_t> m;
    PA_TRY(collect(a, st, m, nullptr));
    uint64_t N = 0, E = 0;
    for (const auto &kv : m) N += kv.second, E += kv.first.size();
    if (N == 0 || G == 0) return PA_OK;
    // the classes (CSR) and their transpose: per-class host work, once per estimate
    ClassTables t;
    t.build(m, G);
    const uint32_t nc = t.nc;
    const std::vector<uint64_t> &c_off = t.c_off, &t_off = t.t_off;
    const std::vector<uint32_t> &c_g = t.c_g, &t_c = t.t_c;
    std::vector<double> n_c(t.n.begin(), t.n.end()), theta0(G, 1.0 / (double)G);
    Bufs b(st);
    uint64_t *d_c_off = nullptr, *d_t_off = nullptr;
    uint32_t *d_c_g = nullptr, *d_t_c = nullptr;
    double *d_n_c = nullptr, *d_len = nullptr, *d_theta[2] = {nullptr, nullptr}, *d_d = nullptr, *d_diff = nullptr,
           *d_delta = nullptr;
    PA_HIP(b.get(&d_c_off, c_off.size() * 8));
    PA_HIP(b.get(&d_t_off, t_off.size() * 8));
    PA_HIP(b.get(&d_c_g, E * 4));
    PA_HIP(b.get(&d_t_c, E * 4));
    PA_HIP(b.get(&d_n_c, (uint64_t)nc * 8));
    PA_HIP(b.get(&d_len, (uint64_t)G * 8));
    PA_HIP(b.get(&d_theta[0], (uint64_t)G * 8));
    PA_HIP(b.get(&d_theta[1], (uint64_t)G * 8));
    PA_HIP(b.get(&d_d, (uint64_t)nc * 8));
    PA_HIP(b.get(&d_diff, (uint64_t)G * 8));
    PA_HIP(b.get(&d_delta, 8));
    PA_HIP(hipMemcpyAsync(d_c_off, c_off.data(), c_off.size() * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_t_off, t_off.data(), t_off.size() * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_c_g, c_g.data(), E * 4, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_t_c, t_c.data(), E * 4, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_n_c, n_c.data(), (uint64_t)nc * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_len, a->h_len.data(), (uint64_t)G * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_theta[0], theta0.data(), (uint64_t)G * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipStreamSynchronize(st));  // (the host vectors above are pageable)
    const unsigned grid_c = (nc + kBlock - 1) / kBlock, grid_g = (G + kBlock - 1) / kBlock;
    uint32_t it = 0;
    int cur = 0;
    double delta = 0;
    while (it < max_iterations) {
        hipLaunchKernelGGL(k_em_e, dim3(grid_c), dim3(kBlock), 0, st, d_c_off, d_c_g, nc, d_theta[cur], d_len, d_d);
        hipLaunchKernelGGL(k_em_m, dim3(grid_g), dim3(kBlock), 0, st, d_t_off, d_t_c, G, d_theta[cur], d_len, d_n_c, d_d,
                           (double)N, d_theta[cur ^ 1], d_diff);
        hipLaunchKernelGGL(k_em_delta, dim3(1), dim3(kBlock), 0, st, d_diff, G, d_delta);
        PA_HIP(hipGetLastError());
        cur ^= 1;
        it++;
        if (tolerance > 0) {  // the one 8-byte copy of an iteration
            PA_HIP(hipMemcpyAsync(&delta, d_delta, 8, hipMemcpyDeviceToHost, st));
            PA_HIP(hipStreamSynchronize(st));
            if (delta < tolerance) break;
        }
    }
    std::vector<double> theta(G);
    PA_HIP(hipMemcpyAsync(&delta, d_delta, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(theta.data(), d_theta[cur], (uint64_t)G * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (read_fraction) std::copy(theta.begin(), theta.end(), read_fraction);
    if (abundance) {
        double sum = 0;
        for (uint32_t g = 0; g < G; g++) sum += rho_of(theta[g], a->h_len[g]);
        for (uint32_t g = 0; g < G; g++) abundance[g] = sum != 0 ? rho_of(theta[g], a->h_len[g]) / sum : 0.0;
    }
    if (iterations_done) *iterations_done = it;
    if (last_delta) *last_delta = delta;
    return PA_OK;
}

pa_status abundance_bootstrap(const pa_abundance *a, uint32_t replicates, uint64_t seed, uint32_t max_iterations,
                              double tolerance, uint64_t *counts, double *read_fraction, double *abundance,
                              uint32_t *iterations, double *last_delta, hipStream_t st) {
    const uint32_t G = a->n_genomes, B = replicates;
    std::map<std::vector<uint32_t>, uint64_t> m;
    PA_TRY(collect(a, st, m, nullptr));
    const uint64_t n_classes = m.size();
    if (counts) std::fill(counts, counts + (uint64_t)B * n_classes, (uint64_t)0);
    if (read_fraction) std::fill(read_fraction, read_fraction + (uint64_t)B * G, 0.0);
    if (abundance) std::fill(abundance, abundance + (uint64_t)B * G, 0.0);
    if (iterations) std::fill(iterations, iterations + B, 0u);
    if (last_delta) std::fill(last_delta, last_delta + B, 0.0);
    uint64_t N = 0;
    for (const auto &kv : m) N += kv.second;
    if (N == 0 || G == 0) return PA_OK;
    ClassTables t;
    t.build(m, G);
    const uint32_t nc = t.nc;
    const uint64_t E = t.c_g.size();
    std::vector<uint64_t> cum((size_t)nc + 1, 0);
    for (uint32_t c = 0; c < nc; c++) cum[c + 1] = cum[c] + t.n[c];
    Bufs b(st);
    uint64_t *d_c_off = nullptr, *d_t_off = nullptr, *d_cum = nullptr;
    uint32_t *d_c_g = nullptr, *d_t_c = nullptr, *d_it = nullptr;
    unsigned long long *d_cnt = nullptr;
    double *d_len = nullptr, *d_theta = nullptr, *d_d = nullptr, *d_out = nullptr, *d_delta = nullptr;
    PA_HIP(b.get(&d_c_off, t.c_off.size() * 8));
    PA_HIP(b.get(&d_t_off, t.t_off.size() * 8));
    PA_HIP(b.get(&d_c_g, E * 4));
    PA_HIP(b.get(&d_t_c, E * 4));
    PA_HIP(b.get(&d_cum, cum.size() * 8));
    PA_HIP(b.get(&d_len, (uint64_t)G * 8));
    PA_HIP(b.get(&d_cnt, (uint64_t)B * nc * 8));
    PA_HIP(b.get(&d_d, (uint64_t)B * nc * 8));
    PA_HIP(b.get(&d_theta, (uint64_t)B * 2 * G * 8));
    PA_HIP(b.get(&d_out, (uint64_t)B * G * 8));
    PA_HIP(b.get(&d_it, (uint64_t)B * 4));
    PA_HIP(b.get(&d_delta, (uint64_t)B * 8));
    PA_HIP(hipMemcpyAsync(d_c_off, t.c_off.data(), t.c_off.size() * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_t_off, t.t_off.data(), t.t_off.size() * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_c_g, t.c_g.data(), E * 4, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_t_c, t.t_c.data(), E * 4, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_cum, cum.data(), cum.size() * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemcpyAsync(d_len, a->h_len.data(), (uint64_t)G * 8, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemsetAsync(d_cnt, 0, (uint64_t)B * nc * 8, st));
    PA_HIP(hipStreamSynchronize(st));  // (the host vectors above are pageable)
    // the draws: a thread takes 64 of them or more, 256 blocks a replicate at most -- and as many as keep a
    // block's draws under 2^31
    const bool lds = nc <= kBootLdsClasses && !pa::env_is("PA_BOOT_LDS", '0');
    const uint64_t per_block = (uint64_t)kBlock * 64;
    const unsigned gx = (unsigned)std::max<uint64_t>(std::min<uint64_t>((N + per_block - 1) / per_block, 256),
                                                     (N + kBootBlockDraws - 1) / kBootBlockDraws);
    if (lds)
        hipLaunchKernelGGL(k_boot_draw<true>, dim3(gx, B), dim3(kBlock), boot_lds_bytes(nc), st, d_cum, nc, N, seed,
                           d_cnt);
    else
        hipLaunchKernelGGL(k_boot_draw<false>, dim3(gx, B), dim3(kBlock), 0, st, d_cum, nc, N, seed, d_cnt);
    PA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_boot_em, dim3(B), dim3(kBlock), 0, st, d_c_off, d_c_g, d_t_off, d_t_c, nc, G, d_len, d_cnt,
                       (double)N, max_iterations, tolerance, d_d, d_theta, d_out, d_it, d_delta);
    PA_HIP(hipGetLastError());
    std::vector<double> theta((size_t)B * G);
    if (counts) PA_HIP(hipMemcpyAsync(counts, d_cnt, (uint64_t)B * nc * 8, hipMemcpyDeviceToHost, st));
    if (iterations) PA_HIP(hipMemcpyAsync(iterations, d_it, (uint64_t)B * 4, hipMemcpyDeviceToHost, st));
    if (last_delta) PA_HIP(hipMemcpyAsync(last_delta, d_delta, (uint64_t)B * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(theta.data(), d_out, theta.size() * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (read_fraction) std::copy(theta.begin(), theta.end(), read_fraction);
    if (abundance)
        for (uint32_t r = 0; r < B; r++) {
            const double *th = theta.data() + (size_t)r * G;
            double *out = abundance + (size_t)r * G;
            double sum = 0;
            for (uint32_t g = 0; g < G; g++) sum += rho_of(th[g], a->h_len[g]);
            for (uint32_t g = 0; g < G; g++) out[g] = sum != 0 ? rho_of(th[g], a->h_len[g]) / sum : 0.0;
        }
    return PA_OK;
}

}  // namespace pa
