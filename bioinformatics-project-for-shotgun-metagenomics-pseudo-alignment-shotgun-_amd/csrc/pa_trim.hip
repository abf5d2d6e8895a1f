// pa_trim.hip -- read trimming on the device: quality ends, then a 3' adapter
// (pa_reads_trim and the per-window pass of the pa_*_fastq_*_ex streams).
// DESIGN.md section 22.
//
//   k_trim_bounds   one wave per read, grid-stride: the two running-sum scans
//                   over the read's quality bytes in chunks of 64 (a wave prefix
//                   scan with the carry taken across chunks; the stop is a
//                   ballot + find-first, the first maximum a wave reduction and
//                   a second ballot), then the adapter search over the bases the
//                   quality step left: every chunk of 64 bases becomes three
//                   64-bit ballots (two code bit planes, one validity plane), a
//                   lane's candidate p is those planes shifted by p, and its
//                   mismatches are one XOR + OR + popcount against the adapter's
//                   planes.  Chunks ascend; the first with a hit ends the search.
//                   No buffer depends on the read length.  start, end and the new
//                   length per read; the statistics with one atomic per block
//                   and counter.
//   offsets         an exclusive 64-bit scan of the new lengths (rocPRIM)
//   k_trim_gather   one thread per 16 aligned OUTPUT bytes of both columns: the
//                   read that holds them is searched in the new offsets (the
//                   block's own range, found once per block), the source bytes
//                   come as two aligned 16-byte loads shifted into place; chunks
//                   that cross a read's end go byte by byte
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "pa_device.h"
#include "pa_internal.h"

using namespace pad;

namespace {

constexpr int kBlock = 256;
// the counters of one pass: pa_trim_stats' nine, the longest and the shortest new read
constexpr int kStat = 9, kMaxLen = 9, kMinLen = 10, kCnt = pa::kTrimCounters;
static_assert(kCnt == 11, "k_trim_bounds' counters");
static_assert(sizeof(pa_trim_stats) == kStat * 8, "pa_trim_stats is nine 64-bit sums");

struct Widen {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

__device__ __forceinline__ int32_t wave_max(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// The running-sum scan of one end: scan position j reads q[rev ? L - 1 - j : j]
// and adds thr - that byte.  The scan stops at the first negative prefix sum;
// the answer is 1 + the first position before the stop that attains the
// largest positive sum (the bases to cut off this end), or 0.  Wave-uniform.
__device__ __forceinline__ uint32_t quality_scan(const uint8_t *__restrict__ q, uint32_t L, int32_t thr, bool rev) {
    const int lane = lane_id();
    int64_t carry = 0, best = 0;
    uint32_t cut = 0;
    for (uint32_t c = 0; c < L; c += 64) {
        const uint32_t j = c + (uint32_t)lane;
        const bool act = j < L;
        const int32_t v = act ? thr - (int32_t)q[rev ? L - 1 - j : j] : 0;
        const int32_t inc = (int32_t)wave_incl_scan((uint32_t)v);  // (two's complement; |inc| <= 64 * 255)
        const uint64_t neg = __ballot(act && carry + inc < 0);
        const int stop = neg ? __ffsll((unsigned long long)neg) - 1 : 64;
        const bool elig = act && lane < stop;
        const int32_t m = wave_max(elig ? inc : INT_MIN);
        if (m != INT_MIN && carry + m > best) {  // (strict: an equal later sum does not move the cut)
            best = carry + m;
            const uint64_t at = __ballot(elig && inc == m);
            cut = c + (uint32_t)__ffsll((unsigned long long)at);
        }
        if (neg) break;
        carry += __shfl(inc, 63);
    }
    return cut;
}

struct Planes {
    uint64_t b0, b1, v;
};

// 64 bases of s from position c as bit planes (bit i: base c + i): the code
// (byte >> 1) & 3 of A, C, G, T (0, 1, 3, 2) and whether the byte is one of them.
__device__ __forceinline__ Planes load_planes(const uint8_t *__restrict__ s, uint32_t c, uint32_t n) {
    const uint32_t p = c + (uint32_t)lane_id();
    const uint32_t b = p < n ? s[p] : 0u;
    const bool ok = b == 'A' || b == 'C' || b == 'G' || b == 'T';
    Planes w;
    w.b0 = __ballot(ok && (b & 2u));
    w.b1 = __ballot(ok && (b & 4u));
    w.v = __ballot(ok);
    return w;
}

__device__ __forceinline__ uint64_t shifted(uint64_t lo, uint64_t hi, int sh) {
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// The smallest hit p of the adapter in s[0, n), or n.  Wave-uniform.
__device__ __forceinline__ uint32_t adapter_find(const uint8_t *__restrict__ s, uint32_t n, const pa::TrimSpec &t) {
    const int lane = lane_id();
    Planes cur = load_planes(s, 0, n);
    for (uint32_t c = 0; c < n; c += 64) {
        Planes nxt{0, 0, 0};
        if (c + 64 < n) nxt = load_planes(s, c + 64, n);
        const uint32_t p = c + (uint32_t)lane;
        bool hit = false;
        if (p < n) {
            const uint32_t ov = min(n - p, t.alen);
            const uint64_t mask = ov >= 64 ? ~0ull : (1ull << ov) - 1;
            const uint64_t r0 = shifted(cur.b0, nxt.b0, lane), r1 = shifted(cur.b1, nxt.b1, lane),
                           rv = shifted(cur.v, nxt.v, lane);
            const uint32_t mm = (uint32_t)__popcll(((r0 ^ t.a0) | (r1 ^ t.a1) | ~rv) & mask);
            hit = ov >= t.min_ov && 1000u * mm <= t.permille * ov;
        }
        const uint64_t h = __ballot(hit);
        if (h) return c + (uint32_t)__ffsll((unsigned long long)h) - 1;
        cur = nxt;
    }
    return n;
}

__global__ __launch_bounds__(kBlock) void k_trim_bounds(const uint8_t *__restrict__ seq,
                                                        const uint8_t *__restrict__ qual,
                                                        const uint64_t *__restrict__ off, uint64_t n,
                                                        const pa::TrimSpec t, uint32_t *__restrict__ start,
                                                        uint32_t *__restrict__ end, uint32_t *__restrict__ len,
                                                        unsigned long long *cnt) {
    __shared__ unsigned long long s_cnt[kCnt];
    if (threadIdx.x < kCnt) s_cnt[threadIdx.x] = threadIdx.x == kMinLen ? ~0ull : 0ull;
    __syncthreads();
    const int lane = lane_id();
    const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / 64);
    uint64_t reads = 0, b_in = 0, b_out = 0, r_trim = 0, r_q = 0, b_q = 0, r_a = 0, b_a = 0, r_empty = 0;
    uint32_t mx = 0, mn = 0xFFFFFFFFu;
    for (uint64_t r = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); r < n; r += nwaves) {
        const uint64_t o = off[r];
        const uint32_t L = (uint32_t)(off[r + 1] - o);
        uint32_t cut = L, st = 0;
        if (t.flags & PA_TRIM_QUALITY3) cut = L - quality_scan(qual + o, L, (int32_t)t.q3, true);
        if (t.flags & PA_TRIM_QUALITY5) st = quality_scan(qual + o, L, (int32_t)t.q5, false);
        if (st >= cut) st = cut = 0;
        uint32_t en = cut;
        if ((t.flags & PA_TRIM_ADAPTER) && cut > st) en = st + adapter_find(seq + o + st, cut - st, t);
        const uint32_t nl = en - st;
        if (lane == 0) {
            start[r] = st;
            end[r] = en;
            len[r] = nl;
        }
        const uint32_t bq = L - (cut - st), ba = cut - en;
        reads++;
        b_in += L;
        b_out += nl;
        r_trim += nl != L;
        r_q += bq != 0;
        b_q += bq;
        r_a += ba != 0;
        b_a += ba;
        r_empty += nl == 0;
        mx = max(mx, nl);
        mn = min(mn, nl);
    }
    if (lane == 0 && reads) {
        const uint64_t mine[kStat] = {reads, b_in, b_out, r_trim, r_q, b_q, r_a, b_a, r_empty};
#pragma unroll
        for (int k = 0; k < kStat; k++)
            if (mine[k]) atomicAdd(&s_cnt[k], (unsigned long long)mine[k]);
        atomicMax(&s_cnt[kMaxLen], (unsigned long long)mx);
        atomicMin(&s_cnt[kMinLen], (unsigned long long)mn);
    }
    __syncthreads();
    if (threadIdx.x < kStat) {
        if (s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_cnt[threadIdx.x]);
    } else if (threadIdx.x == kMaxLen) {
        if (s_cnt[kMaxLen]) atomicMax(&cnt[kMaxLen], s_cnt[kMaxLen]);
    } else if (threadIdx.x == kMinLen) {
        if (s_cnt[kMinLen] != ~0ull) atomicMin(&cnt[kMinLen], s_cnt[kMinLen]);
    }
}

// The last read r in [a, b] with ooff[r] <= pos (ooff ascending; reads of
// length 0 share their successor's offset, so the last one is the holder).
__device__ __forceinline__ uint64_t read_at(const uint64_t *__restrict__ ooff, uint64_t a, uint64_t b, uint64_t pos) {
    while (a < b) {
        const uint64_t m = (a + b + 1) >> 1;
        if (ooff[m] <= pos) a = m;
        else b = m - 1;
    }
    return a;
}

// The 16 bytes of col from src on: two aligned 16-byte loads shifted into
// place (the second one only when src is not aligned).
__device__ __forceinline__ uint4 load16_at(const uint8_t *__restrict__ col, uint64_t src) {
    const uint64_t a = src & ~15ull;
    const uint32_t sh = (uint32_t)(src & 15);
    const uint4 x = *(const uint4 *)(col + a);
    uint64_t q0 = x.x | ((uint64_t)x.y << 32), q1 = x.z | ((uint64_t)x.w << 32);
    if (sh) {
        const uint4 y = *(const uint4 *)(col + a + 16);
        uint64_t q2 = y.x | ((uint64_t)y.y << 32), q3 = y.z | ((uint64_t)y.w << 32);
        uint32_t s = sh;
        if (s >= 8) q0 = q1, q1 = q2, q2 = q3, s -= 8;
        if (s) {
            const uint32_t bits = 8 * s;
            q0 = (q0 >> bits) | (q1 << (64 - bits));
            q1 = (q1 >> bits) | (q2 << (64 - bits));
        }
    }
    uint4 v;
    v.x = (uint32_t)q0, v.y = (uint32_t)(q0 >> 32), v.z = (uint32_t)q1, v.w = (uint32_t)(q1 >> 32);
    return v;
}

// 16 output bytes of each column per thread, aligned in the outputs (one
// 16-byte store per column, lanes consecutive).  Read r's kept bytes
// [ioff[r] + start[r], + its new length) go to [ooff[r], ooff[r + 1]).  The
// loads stay below the last kept byte's 16-byte block + 16, inside the
// columns' kReadPad; the stores below ooff[n] + 15, inside the outputs'.
__global__ __launch_bounds__(kBlock) void k_trim_gather(const uint8_t *__restrict__ iseq,
                                                        const uint8_t *__restrict__ iqual,
                                                        const uint64_t *__restrict__ ioff,
                                                        const uint32_t *__restrict__ start,
                                                        const uint64_t *__restrict__ ooff, uint64_t n,
                                                        uint8_t *__restrict__ oseq, uint8_t *__restrict__ oqual) {
    __shared__ uint64_t s_rec[2];
    const uint64_t total = ooff[n];
    const uint64_t b0 = (uint64_t)blockIdx.x * kBlock * 16;
    if (b0 >= total) return;  // (the grid covers the input's bases; the whole block leaves)
    if (threadIdx.x < 2) {    // the reads of the block's first and last byte
        const uint64_t p = threadIdx.x == 0 ? b0 : min(total - 1, b0 + kBlock * 16 - 1);
        s_rec[threadIdx.x] = read_at(ooff, 0, n - 1, p);
    }
    __syncthreads();
    const uint64_t pos = b0 + 16 * threadIdx.x;
    if (pos >= total) return;
    uint64_t r = read_at(ooff, s_rec[0], s_rec[1], pos);
    uint64_t o = ooff[r], e = ooff[r + 1];  // (e > pos: r is the holder, of length e - o >= 1)
    uint64_t src = ioff[r] + start[r] + (pos - o);
    uint4 vs, vq;
    if (pos + 16 <= e) {
        vs = load16_at(iseq, src);
        vq = load16_at(iqual, src);
    } else {  // a read's end inside the chunk
        uint64_t w[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int j = 0; j < 16; j++) {
            const uint64_t p = pos + j;
            if (p >= total) break;
            if (p >= e) {  // the next read of length >= 1 (p < total: there is one)
                r = read_at(ooff, r + 1, s_rec[1], p);
                o = ooff[r], e = ooff[r + 1];
                src = ioff[r] + start[r] - j;  // (p == o here)
            }
            const uint64_t cs = iseq[src + j], cq = iqual[src + j];
            const int sh = 8 * (j & 7);
            w[j >> 3] |= cs << sh;
            w[2 + (j >> 3)] |= cq << sh;
        }
        vs.x = (uint32_t)w[0], vs.y = (uint32_t)(w[0] >> 32), vs.z = (uint32_t)w[1], vs.w = (uint32_t)(w[1] >> 32);
        vq.x = (uint32_t)w[2], vq.y = (uint32_t)(w[2] >> 32), vq.z = (uint32_t)w[3], vq.w = (uint32_t)(w[3] >> 32);
    }
    *(uint4 *)(oseq + pos) = vs;
    *(uint4 *)(oqual + pos) = vq;
}

}  // namespace

namespace pa {

pa_status trim_spec_check(const pa_trim_spec *spec, TrimSpec *out) {
    const uint32_t known = PA_TRIM_QUALITY3 | PA_TRIM_QUALITY5 | PA_TRIM_ADAPTER;
    auto bad = [](const char *msg) {
        set_error(std::string("pa_trim_spec: ") + msg);
        return PA_EINVAL;
    };
    if (spec->flags & ~known) return bad("unknown flag bits");
    if (spec->quality3 > 255 || spec->quality5 > 255) return bad("a quality cutoff is a byte, 0 .. 255");
    if (spec->min_overlap == 0) return bad("min_overlap must be at least 1");
    if (spec->max_error_permille > 500) return bad("max_error_permille must be 0 .. 500");
    *out = TrimSpec{};
    out->flags = spec->flags;
    out->q3 = spec->quality3;
    out->q5 = spec->quality5;
    out->min_ov = spec->min_overlap;
    out->permille = spec->max_error_permille;
    if (spec->flags & PA_TRIM_ADAPTER) {
        if (spec->adapter_len == 0 || spec->adapter_len > PA_TRIM_MAX_ADAPTER)
            return bad("adapter_len must be 1 .. PA_TRIM_MAX_ADAPTER");
        out->alen = spec->adapter_len;
        for (uint32_t j = 0; j < spec->adapter_len; j++) {
            const unsigned char c = (unsigned char)spec->adapter[j];
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return bad("an adapter byte outside ACGT");
            out->a0 |= (uint64_t)((c >> 1) & 1u) << j;  // (load_planes' code of the byte)
            out->a1 |= (uint64_t)((c >> 2) & 1u) << j;
        }
    }
    return PA_OK;
}

// The whole pass on the stream, then one wait: d_start / d_end [n], d_len
// [n + 1], o_off [n + 1], o_seq / o_qual [in_bases + kReadPad], d_cnt
// [kTrimCounters] are the caller's; in_bases bounds the input's bases (the
// gather's grid).  stats (nullable) accumulates.
pa_status trim_device(const pa_reads *in, uint64_t in_bases, const TrimSpec &t, uint32_t *d_start, uint32_t *d_end,
                      uint32_t *d_len, uint8_t *o_seq, uint8_t *o_qual, uint64_t *o_off, unsigned long long *d_cnt,
                      Bufs &b, pa_trim_stats *stats, TrimOut *out, hipStream_t st) {
    const uint64_t n = in->n;
    *out = TrimOut{};
    if (n == 0) {
        PA_HIP(hipMemsetAsync(o_off, 0, 8, st));
        return PA_OK;
    }
    unsigned long long h[kCnt];
    for (int k = 0; k < kCnt; k++) h[k] = k == kMinLen ? ~0ull : 0ull;
    // PA_TRIM_TIMING=1: the split of this call (bounds kernel, offset scan, gather kernel) on stderr
    struct Events {
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) hipEventDestroy(x);
        }
    } ev;
    const bool timing = env_is("PA_TRIM_TIMING", '1');
    if (timing)
        for (hipEvent_t &x : ev.e) PA_HIP(hipEventCreate(&x));
    auto mark = [&](int i) { return timing ? hipEventRecord(ev.e[i], st) : hipSuccess; };
    PA_HIP(hipMemcpyAsync(d_cnt, h, sizeof h, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemsetAsync(d_len + n, 0, 4, st));
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock / 64 - 1) / (kBlock / 64), 8192));
    PA_HIP(mark(0));
    hipLaunchKernelGGL(k_trim_bounds, dim3(grid), dim3(kBlock), 0, st, in->seq, in->qual, in->off, n, t, d_start,
                       d_end, d_len, d_cnt);
    PA_HIP(hipGetLastError());
    PA_HIP(mark(1));
    auto len64 = rocprim::make_transform_iterator(d_len, Widen{});
    PA_HIP(with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, len64, o_off, (uint64_t)0, (size_t)(n + 1),
                                       rocprim::plus<uint64_t>(), st);
    }));
    PA_HIP(mark(2));
    if (in_bases) {
        hipLaunchKernelGGL(k_trim_gather, dim3((unsigned)((in_bases + kBlock * 16 - 1) / (kBlock * 16))), dim3(kBlock),
                           0, st, in->seq, in->qual, in->off, d_start, o_off, n, o_seq, o_qual);
        PA_HIP(hipGetLastError());
    }
    PA_HIP(mark(3));
    PA_HIP(hipMemcpyAsync(h, d_cnt, sizeof h, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (timing) {
        float ms[3] = {0, 0, 0};
        for (int i = 0; i < 3; i++) hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]);
        fprintf(stderr, "[pa_trim] %llu reads, %llu bases in, %llu out: bounds %.3f ms, offsets %.3f ms, gather %.3f ms\n",
                (unsigned long long)n, h[1], h[2], ms[0], ms[1], ms[2]);
    }
    if (h[0] != n || h[1] > in_bases) {
        set_error(std::string(err_op()) + ": the trim pass counted other reads or bases than the batch holds "
                                          "(invariant violated)");
        return PA_EINTERNAL;
    }
    out->n_bases = h[2];
    out->max_len = (uint32_t)h[kMaxLen];
    out->len_min = (int64_t)h[kMinLen];
    if (stats)  // (the counters' order is k_trim_bounds' `mine`)
        trim_stats_add(stats, pa_trim_stats{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8]});
    return PA_OK;
}

// pa_reads_trim: a new batch, start / end to the host when wanted.
pa_status reads_trim(const pa_reads *in, const TrimSpec &t, pa_reads *out, uint32_t *start, uint32_t *end,
                     pa_trim_stats *stats, hipStream_t st) {
    ErrOp op("pa_reads_trim");
    const uint64_t n = in->n;
    out->device = in->device;
    out->n = n;
    PA_HIP(dev_malloc(&out->seq, in->n_bases + kReadPad));
    PA_HIP(dev_malloc(&out->qual, in->n_bases + kReadPad));
    PA_HIP(dev_malloc(&out->off, (n + 1) * 8));
    Bufs b(st);
    uint32_t *d_start = nullptr, *d_end = nullptr, *d_len = nullptr;
    unsigned long long *d_cnt = nullptr;
    PA_HIP(b.get(&d_start, n * 4));
    PA_HIP(b.get(&d_end, n * 4));
    PA_HIP(b.get(&d_len, (n + 1) * 4));
    PA_HIP(b.get(&d_cnt, kTrimCounters * 8));
    TrimOut to;
    PA_TRY(trim_device(in, in->n_bases, t, d_start, d_end, d_len, out->seq, out->qual, out->off, d_cnt, b, stats, &to,
                       st));
    out->n_bases = to.n_bases;
    out->max_len = to.max_len;
    out->q_min = in->q_min < 0 ? -1 : in->q_min;  // (a lower bound of the kept bytes too; -1: effective_params measures)
    out->len_min = to.len_min;                     // (measured by k_trim_bounds, whatever in's state)
    if (n && start) PA_HIP(hipMemcpyAsync(start, d_start, n * 4, hipMemcpyDeviceToHost, st));
    if (n && end) PA_HIP(hipMemcpyAsync(end, d_end, n * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

}  // namespace pa
