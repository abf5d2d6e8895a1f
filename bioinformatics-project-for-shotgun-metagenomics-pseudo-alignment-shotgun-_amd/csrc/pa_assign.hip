// pa_assign.hip -- the assign pass: which genome(s) each read of a batch
// belongs to (pa_align_detail's outputs, bit for bit) at the cost of the
// counter pass plus a small remainder.  DESIGN.md section 11.
//
//   classify   the lane kernels' AS instantiations (pa_lane.h, lane_assign)
//              store, for every read they settle, its type, list length (0 or
//              1), genome, filtered_kmers and redundant_kmers at the read's
//              batch-local number; the reads they leave -- queue_hard -- are
//              walked by k_align_exact in detail mode over that queue.  The
//              wave kernel is not launched (it keeps no per-read detail).
//              Without a lane path (k > 95, no tiles, PA_NO_LANE=1, PA_ASSIGN=0)
//              every read goes to the exact kernel, as pa_align_detail does it.
//   offsets    an exclusive scan of the list lengths, on the device.
//   lists      k_assign_scatter writes the one-entry lists of the lane-settled
//              reads at their offsets, the exact kernel's second pass over the
//              same queue writes the rest.
//   cover      the type array starts as kAssignUnset; a count of the reads still
//              holding it after the last kernel must be zero (PA_EINTERNAL).
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

// The one-entry lists of the reads a lane kernel settled as unique (g[i] set);
// the exact kernel writes its own reads' lists (their g[i] stays unset).
__global__ __launch_bounds__(kBlock) void k_assign_scatter(const uint32_t *__restrict__ g,
                                                           const uint64_t *__restrict__ off, uint64_t n,
                                                           uint64_t total, uint32_t *__restrict__ lists) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t v = g[i];
        if (v == pa::kAssignNoGenome) continue;
        const uint64_t o = off[i];
        if (o < total) lists[o] = v;
    }
}

// Reads no kernel settled: one atomic per block.
__global__ __launch_bounds__(kBlock) void k_assign_unset(const uint8_t *__restrict__ type, uint64_t n,
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

inline uint64_t up16(uint64_t b) { return (b + 15) / 16 * 16; }

}  // namespace

namespace pa {

pa_status assign_pass_device(pa_index *idx, const pa_reads *r, const DevParams &p, uint64_t list_cap, AssignDev &out,
                             Bufs &b, hipStream_t st) {
    out = AssignDev{};
    const uint64_t n = r->n;
    if (n == 0) return PA_OK;
    if (n >= 0xFFFFFFFFull) {
        set_error("pa_align_reads: a batch holds at most 2^32 - 2 reads (split it)");
        return PA_EUNSUPPORTED;
    }
    const uint64_t G = idx->n_genomes;
    // one allocation: off [n + 1] | qf [n] | hr [n] | len [n + 1] | g [n] | type [n] | scratch | unset count
    const uint64_t b_off = 0, b_qf = b_off + up16((n + 1) * 8), b_hr = b_qf + up16(n * 4), b_len = b_hr + up16(n * 4),
                   b_g = b_len + up16((n + 1) * 4), b_type = b_g + n * 4, b_scr = up16(b_type + n),
                   b_cnt = b_scr + up16((6 + 3 * G) * 8), bytes = b_cnt + 16;
    unsigned char *blk = nullptr;
    PA_HIP(b.get(&blk, bytes));
    out.off = (uint64_t *)(blk + b_off);
    out.qf = (uint32_t *)(blk + b_qf);
    out.hr = (uint32_t *)(blk + b_hr);
    out.len = (uint32_t *)(blk + b_len);
    out.type = blk + b_type;
    AssignBufs as{};
    as.type = out.type;
    as.qf = out.qf;
    as.hr = out.hr;
    as.len = out.len;
    as.g = (uint32_t *)(blk + b_g);
    as.scratch = blk + b_scr;
    as.lane = !pa::env_is("PA_ASSIGN", '0');
    unsigned long long *d_cnt = (unsigned long long *)(blk + b_cnt);
    // g and type (adjacent) unset; the scratch counters and the count zero; len[n] = 0 (the scan's last input)
    PA_HIP(hipMemsetAsync(blk + b_g, 0xFF, n * 5, st));
    PA_HIP(hipMemsetAsync(blk + b_scr, 0, b_cnt + 16 - b_scr, st));
    PA_HIP(hipMemsetAsync(out.len + n, 0, 4, st));
    bool queued = false;
    PA_TRY(assign_classify(idx, r, p, as, &queued, st));
    // list offsets: a device scan of the list lengths, widened on the fly
    auto len64 = rocprim::make_transform_iterator(out.len, Widen{});
    PA_HIP(with_temp(b, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, len64, out.off, (uint64_t)0, (size_t)(n + 1),
                                       rocprim::plus<uint64_t>(), st);
    }));
    uint64_t total = 0;
    PA_HIP(hipMemcpyAsync(&total, out.off + n, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    out.total = total;
    if (total > 0 && total <= list_cap) {
        PA_HIP(b.get(&out.lists, total * 4));
        if (queued) {
            hipLaunchKernelGGL(k_assign_scatter, dim3(grid_for(n)), dim3(kBlock), 0, st, as.g, out.off, n, total,
                               out.lists);
            PA_HIP(hipGetLastError());
        }
        PA_TRY(assign_lists(idx, r, p, as, queued, out.off, out.lists, st));
    }
    // every read settled by exactly one kernel -- at least by one: none still unset
    hipLaunchKernelGGL(k_assign_unset, dim3(std::min(grid_for(n), 2048u)), dim3(kBlock), 0, st, out.type, n, d_cnt);
    PA_HIP(hipGetLastError());
    unsigned long long unset = 0;
    PA_HIP(hipMemcpyAsync(&unset, d_cnt, 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (unset) {
        set_error("pa_align_reads: " + std::to_string(unset) + " reads were settled by no kernel (invariant violated)");
        return PA_EINTERNAL;
    }
    return PA_OK;
}

pa_status align_reads(pa_index *idx, const pa_reads *r, const DevParams &p, uint8_t *type, uint32_t *qf, uint32_t *hr,
                      uint64_t *list_off, uint32_t *lists, uint64_t list_cap, uint64_t *list_total, hipStream_t st) {
    const uint64_t n = r->n;
    list_off[0] = 0;
    *list_total = 0;
    if (n == 0) return PA_OK;
    if (!lists) list_cap = 0;
    Bufs b(st);
    AssignDev d;
    PA_TRY(assign_pass_device(idx, r, p, list_cap, d, b, st));
    PA_HIP(hipMemcpyAsync(type, d.type, n, hipMemcpyDeviceToHost, st));
    if (qf) PA_HIP(hipMemcpyAsync(qf, d.qf, n * 4, hipMemcpyDeviceToHost, st));
    if (hr) PA_HIP(hipMemcpyAsync(hr, d.hr, n * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(list_off, d.off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (d.lists) PA_HIP(hipMemcpyAsync(lists, d.lists, d.total * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    *list_total = d.total;
    if (d.total > list_cap) {
        set_error("pa_align_reads: list_cap smaller than the required list length");
        return PA_EINVAL;
    }
    return PA_OK;
}

}  // namespace pa
