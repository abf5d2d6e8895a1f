// pa_extract.hip -- read extraction: the selected FASTQ records of a window
// gathered on the device (pa_extract_fastq_file) and the selection flags of an
// uploaded batch (pa_reads_select).  DESIGN.md section 20.
//
//   classify          the assign pass (pa_assign.hip) leaves every read's type
//                     and genome list on the device
//   k_extract_select  one thread per record: sel(r), the record's output
//                     length (0, or its bytes + the closing line feed), the
//                     selected records per type (ballots per wave, four
//                     integer atomics per block)
//   offsets           an exclusive 64-bit scan of the lengths (rocPRIM)
//   k_extract_gather  one thread per 16 aligned OUTPUT bytes: the record that
//                     holds them is searched in the offsets (the block's own
//                     range of records, found once per block), the source
//                     bytes come as two aligned 16-byte loads shifted into
//                     place; chunks that cross a record's end, or whose second
//                     load would touch the window's end, go byte by byte
//   write out         one device-to-host copy into pinned memory, one write loop
#include <errno.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <string>

#include "pa_device.h"
#include "pa_internal.h"

using namespace pad;

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kTypeBits = (1u << PA_DROPPED) | (1u << PA_UNMAPPED) | (1u << PA_UNIQUELY_MAPPED) |
                               (1u << PA_AMBIGUOUSLY_MAPPED);

struct Widen {
    __host__ __device__ uint64_t operator()(uint32_t v) const { return v; }
};

// sel(r) per record; with nl (the window's line-feed offsets, relative to t0)
// the record's output length too: qe - hs + 1, hs and qe as k_records has them.
__global__ __launch_bounds__(kBlock) void k_extract_select(const uint8_t *__restrict__ type,
                                                           const uint64_t *__restrict__ off,
                                                           const uint32_t *__restrict__ lists,
                                                           const uint8_t *__restrict__ keep, uint32_t type_mask,
                                                           uint32_t invert, uint64_t n, const uint32_t *__restrict__ nl,
                                                           uint64_t t0, uint64_t lo, uint32_t *__restrict__ out_len,
                                                           uint8_t *__restrict__ flag, unsigned long long *by_type) {
    __shared__ uint32_t s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mine[4] = {0, 0, 0, 0};
    // (whole waves run every round: the ballots below take every lane)
    const uint64_t rounds = (n + (uint64_t)gridDim.x * kBlock - 1) / ((uint64_t)gridDim.x * kBlock);
    for (uint64_t it = 0; it < rounds; it++) {
        const uint64_t r = (it * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        bool sel = false;
        uint32_t t = 0;
        if (r < n) {
            t = type[r];
            sel = t < 4 && ((type_mask >> t) & 1u);
            if (sel && keep && (t == PA_UNIQUELY_MAPPED || t == PA_AMBIGUOUSLY_MAPPED)) {
                bool any = false;
                for (uint64_t j = off[r], e = off[r + 1]; j < e && !any; j++) any = keep[lists[j]] != 0;
                sel = any;
            }
            if (invert) sel = !sel;
            if (nl) {
                const uint64_t hs = r ? t0 + nl[4 * r - 1] + 1 : lo, qe = t0 + nl[4 * r + 3];
                out_len[r] = sel ? (uint32_t)(qe - hs + 1) : 0u;
            }
            if (flag) flag[r] = sel ? 1 : 0;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint64_t b = __ballot(sel && t == k);
            if (lane_id() == 0) mine[k] += (uint32_t)__popcll(b);
        }
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (mine[k]) atomicAdd(&s_cnt[k], mine[k]);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&by_type[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// The last record r in [a, b] with ooff[r] <= pos (ooff ascending; records of
// length 0 share their successor's offset, so the last one is the holder).
__device__ __forceinline__ uint64_t rec_at(const uint64_t *__restrict__ ooff, uint64_t a, uint64_t b, uint64_t pos) {
    while (a < b) {
        const uint64_t m = (a + b + 1) >> 1;
        if (ooff[m] <= pos) a = m;
        else b = m - 1;
    }
    return a;
}

// 16 output bytes per thread, aligned in `out` (one 16-byte store, lanes
// consecutive).  ooff[R + 1]: the records' output offsets and the total.  A
// selected record r holds the output bytes [ooff[r], ooff[r + 1]): its text
// D[hs, qe) and a line feed written here (D[qe] is none for a last record
// without one).  No byte of D at or past hi is read.
__global__ __launch_bounds__(kBlock) void k_extract_gather(const uint8_t *__restrict__ D, uint64_t t0, uint64_t lo,
                                                           uint64_t hi, const uint32_t *__restrict__ nl,
                                                           const uint64_t *__restrict__ ooff, uint64_t R,
                                                           uint64_t total, uint8_t *__restrict__ out) {
    __shared__ uint64_t s_rec[2];
    const uint64_t b0 = (uint64_t)blockIdx.x * kBlock * 16;
    if (threadIdx.x < 2) {  // the records of the block's first and last byte
        const uint64_t p = threadIdx.x == 0 ? b0 : min(total - 1, b0 + kBlock * 16 - 1);
        s_rec[threadIdx.x] = rec_at(ooff, 0, R - 1, p);
    }
    __syncthreads();
    const uint64_t pos = b0 + 16 * threadIdx.x;
    if (pos >= total) return;
    uint64_t r = rec_at(ooff, s_rec[0], s_rec[1], pos);
    uint64_t o = ooff[r], e = ooff[r + 1];  // (e > pos: r is the holder, of length e - o >= 1)
    uint64_t hs = r ? t0 + nl[4 * r - 1] + 1 : lo;
    uint64_t w0, w1;
    const uint64_t src = hs + (pos - o);
    const uint64_t a = src & ~15ull;
    const uint32_t sh = (uint32_t)(src & 15);
    if (pos + 16 < e && a + (sh ? 32 : 16) <= hi) {  // 16 text bytes of one record, both loads below hi
        const uint4 x = *(const uint4 *)(D + a);
        uint64_t q0 = x.x | ((uint64_t)x.y << 32), q1 = x.z | ((uint64_t)x.w << 32);
        if (sh) {
            const uint4 y = *(const uint4 *)(D + a + 16);
            uint64_t q2 = y.x | ((uint64_t)y.y << 32), q3 = y.z | ((uint64_t)y.w << 32);
            uint32_t s = sh;
            if (s >= 8) q0 = q1, q1 = q2, q2 = q3, s -= 8;
            if (s) {
                const uint32_t bits = 8 * s;
                q0 = (q0 >> bits) | (q1 << (64 - bits));
                q1 = (q1 >> bits) | (q2 << (64 - bits));
            }
        }
        w0 = q0, w1 = q1;
    } else {  // a record's end (or the text's) inside the chunk
        w0 = w1 = 0;
#pragma unroll 1
        for (int j = 0; j < 16; j++) {
            const uint64_t p = pos + j;
            if (p >= total) break;
            if (p >= e) {  // the next selected record (p < total: there is one)
                r = rec_at(ooff, r + 1, s_rec[1], p);
                o = ooff[r], e = ooff[r + 1];
                hs = t0 + nl[4 * r - 1] + 1;
            }
            const uint64_t c = p + 1 == e ? (uint64_t)'\n' : (uint64_t)D[hs + (p - o)];
            if (j < 8) w0 |= c << (8 * j);
            else w1 |= c << (8 * (j - 8));
        }
    }
    uint4 v;
    v.x = (uint32_t)w0, v.y = (uint32_t)(w0 >> 32), v.z = (uint32_t)w1, v.w = (uint32_t)(w1 >> 32);
    *(uint4 *)(out + pos) = v;
}

inline unsigned grid_for(uint64_t n) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, 65536));
}

pa_status write_all(int fd, const uint8_t *p, uint64_t n) {
    while (n) {
        const ssize_t w = write(fd, p, (size_t)std::min<uint64_t>(n, 1u << 30));
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) {
            pa::set_error(std::string("pa_extract_fastq_file: write failed") +
                          (w < 0 ? std::string(": ") + strerror(errno) : std::string(" (short write)")));
            return PA_EIO;
        }
        p += w;
        n -= (uint64_t)w;
    }
    return PA_OK;
}

}  // namespace

namespace pa {

bool extract_mask_ok(uint32_t type_mask) { return type_mask != 0 && (type_mask & ~kTypeBits) == 0; }

pa_status extract_open(Extract &x, const pa_index *idx, const pa_extract_spec *spec, int fd, uint64_t span,
                       pa_extract_stats *stats, hipStream_t st) {
    x.type_mask = spec->type_mask;
    x.invert = (spec->flags & PA_EXTRACT_INVERT) ? 1u : 0u;
    x.fd = fd;
    x.cap = span + 16;
    x.stats = stats;
    x.timing = pa::env_is("PA_STREAM_TIMING", '1');
    PA_HIP(pa::dev_malloc(&x.by_type, 4 * 8));
    PA_HIP(hipMemsetAsync(x.by_type, 0, 4 * 8, st));
    if (spec->genome_keep && idx->n_genomes) {
        PA_HIP(pa::dev_malloc(&x.keep, idx->n_genomes));
        PA_HIP(hipMemcpyAsync(x.keep, spec->genome_keep, idx->n_genomes, hipMemcpyHostToDevice, st));
        PA_HIP(hipStreamSynchronize(st));  // (the caller's array may go after the call that opened)
    }
    PA_HIP(pa::dev_malloc(&x.d_out, x.cap));
    PA_HIP(hipHostMalloc((void **)&x.h_out, x.cap, hipHostMallocDefault));
    for (hipEvent_t &e : x.ev) PA_HIP(hipEventCreate(&e));
    return PA_OK;
}

void extract_close(Extract &x) {
    pa::dev_free(x.by_type);
    pa::dev_free(x.keep);
    pa::dev_free(x.d_out);
    if (x.h_out) hipHostFree(x.h_out);
    for (hipEvent_t &e : x.ev)
        if (e) hipEventDestroy(e);
    x = Extract{};
}

static pa_status launch_select(const Extract &x, const AssignDev &as, uint64_t n, const uint32_t *nl, uint64_t t0,
                               uint64_t lo, uint32_t *d_len, uint8_t *d_flag, hipStream_t st) {
    hipLaunchKernelGGL(k_extract_select, dim3(grid_for(n)), dim3(kBlock), 0, st, as.type, as.off, as.lists, x.keep,
                       x.type_mask, x.invert, n, nl, t0, lo, d_len, d_flag, x.by_type);
    PA_HIP(hipGetLastError());
    return PA_OK;
}

// The selected records of one parsed window (its reads r, its text D[lo, hi)
// and line feeds nl) classified, gathered and written to x.fd.
pa_status extract_window(Extract &x, pa_index *idx, const pa_reads *r, const DevParams &prm, const uint8_t *D,
                         uint64_t t0, uint64_t lo, uint64_t hi, const uint32_t *nl, hipStream_t st) {
    const uint64_t R = r->n;
    if (R == 0) return PA_OK;
    ErrOp op("pa_extract_fastq_file");
    Bufs b(st);
    AssignDev as;
    if (x.timing) PA_HIP(hipEventRecord(x.ev[0], st));
    PA_TRY(assign_pass_device(idx, r, prm, ~0ull, as, b, st));
    if (x.timing) PA_HIP(hipEventRecord(x.ev[1], st));
    uint32_t *d_len = nullptr;
    uint64_t *d_ooff = nullptr;
    PA_HIP(b.get(&d_len, (R + 1) * 4));
    PA_HIP(b.get(&d_ooff, (R + 1) * 8));
    PA_HIP(hipMemsetAsync(d_len + R, 0, 4, st));
    PA_TRY(launch_select(x, as, R, nl, t0, lo, d_len, nullptr, st));
    auto len64 = rocprim::make_transform_iterator(d_len, Widen{});
    PA_HIP(with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, len64, d_ooff, (uint64_t)0, (size_t)(R + 1),
                                       rocprim::plus<uint64_t>(), st);
    }));
    uint64_t total = 0;
    unsigned long long by_type[4];
    PA_HIP(hipMemcpyAsync(&total, d_ooff + R, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(by_type, x.by_type, sizeof by_type, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (total > x.cap - 15) {  // (at most the window's bytes and one added line feed)
        set_error("pa_extract_fastq_file: a window's output is larger than its text (invariant violated)");
        return PA_EINTERNAL;
    }
    float ms_gather = 0, ms_copy = 0;
    double ms_write = 0;
    if (x.timing) PA_HIP(hipEventRecord(x.ev[2], st));
    if (total) {
        hipLaunchKernelGGL(k_extract_gather, dim3((unsigned)((total + kBlock * 16 - 1) / (kBlock * 16))), dim3(kBlock),
                           0, st, D, t0, lo, hi, nl, d_ooff, R, total, x.d_out);
        PA_HIP(hipGetLastError());
        if (x.timing) PA_HIP(hipEventRecord(x.ev[3], st));
        PA_HIP(hipMemcpyAsync(x.h_out, x.d_out, total, hipMemcpyDeviceToHost, st));
        if (x.timing) PA_HIP(hipEventRecord(x.ev[4], st));
        PA_HIP(hipStreamSynchronize(st));
        const auto tw = std::chrono::steady_clock::now();
        PA_TRY(write_all(x.fd, x.h_out, total));
        ms_write = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw).count();
    }
    x.stats->records += R;
    x.stats->bytes += total;
    uint64_t selected = 0;
    for (int k = 0; k < 4; k++) {
        x.stats->selected_by_type[k] = by_type[k];  // (the device counters run over the file)
        selected += by_type[k];
    }
    x.stats->selected = selected;
    if (x.timing) {
        float ms_parse = 0, ms_assign = 0, ms_select = 0;
        if (!total) PA_HIP(hipEventSynchronize(x.ev[2]));
        hipEventElapsedTime(&ms_parse, x.ev[5], x.ev[0]);
        hipEventElapsedTime(&ms_assign, x.ev[0], x.ev[1]);
        hipEventElapsedTime(&ms_select, x.ev[1], x.ev[2]);
        if (total) {
            hipEventElapsedTime(&ms_gather, x.ev[2], x.ev[3]);
            hipEventElapsedTime(&ms_copy, x.ev[3], x.ev[4]);
        }
        fprintf(stderr, "[pa_extract] window: %llu records, %llu text bytes, %llu bytes out: parse + counter pass %.3f "
                        "ms, assign %.3f ms, select + scan %.3f ms, gather %.3f ms, copy to host %.3f ms, write %.3f ms\n",
                (unsigned long long)R, (unsigned long long)(hi - lo), (unsigned long long)total, ms_parse, ms_assign,
                ms_select, ms_gather, ms_copy, ms_write);
    }
    return PA_OK;
}

// sel(r) of an uploaded batch: the assign pass and k_extract_select.
pa_status reads_select(pa_index *idx, const pa_reads *r, const DevParams &prm, const pa_extract_spec *spec,
                       uint8_t *selected, uint64_t *n_selected, hipStream_t st) {
    *n_selected = 0;
    const uint64_t n = r->n;
    if (n == 0) return PA_OK;
    ErrOp op("pa_reads_select");
    Bufs b(st);
    Extract x;
    x.type_mask = spec->type_mask;
    x.invert = (spec->flags & PA_EXTRACT_INVERT) ? 1u : 0u;
    PA_HIP(b.get(&x.by_type, 4 * 8));
    PA_HIP(hipMemsetAsync(x.by_type, 0, 4 * 8, st));
    if (spec->genome_keep && idx->n_genomes) {
        PA_HIP(b.get(&x.keep, idx->n_genomes));
        PA_HIP(hipMemcpyAsync(x.keep, spec->genome_keep, idx->n_genomes, hipMemcpyHostToDevice, st));
    }
    AssignDev as;
    PA_TRY(assign_pass_device(idx, r, prm, ~0ull, as, b, st));
    uint8_t *d_flag = nullptr;
    PA_HIP(b.get(&d_flag, n));
    PA_TRY(launch_select(x, as, n, nullptr, 0, 0, nullptr, d_flag, st));
    unsigned long long by_type[4];
    PA_HIP(hipMemcpyAsync(by_type, x.by_type, sizeof by_type, hipMemcpyDeviceToHost, st));
    if (selected) PA_HIP(hipMemcpyAsync(selected, d_flag, n, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    *n_selected = by_type[0] + by_type[1] + by_type[2] + by_type[3];
    return PA_OK;
}

}  // namespace pa
