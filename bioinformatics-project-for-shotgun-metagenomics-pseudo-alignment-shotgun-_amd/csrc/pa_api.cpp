// extern "C" entry points of libpa.so (declared in include/pa.h).
//
// Argument checks mirror the reference's (src/kmer.py:125-126, 501-510);
// EXTQUALITY thresholds are clamped to ranges where the strict comparisons of
// src/kmer.py:420, 425, 587 keep their meaning, so the kernels can use 32-bit
// arithmetic:
//   mean quality < T  with byte qualities in [0, 255]:  T <= 0 never, T >= 256 always
//   set size > mg     with set sizes in [1, G]:          mg < 0 always, mg >= G never
//   top >= second + m with counts <= windows < 2^31:     m clamped to 2^30
//   max - mapped > p  likewise p clamped to 2^30 (p < 0 keeps "skip")
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "pa_internal.h"

namespace pa {
static thread_local std::string g_err;
static thread_local const char *g_op = nullptr;
void set_error(const std::string &msg) { g_err = msg; }
ErrOp::ErrOp(const char *name) : prev(g_op) { g_op = name; }
ErrOp::~ErrOp() { g_op = prev; }
const char *err_op() { return g_op ? g_op : ""; }
pa_status hip_failed(hipError_t e, const char *where) {
    (void)hipGetLastError();
    set_error((g_op ? std::string(g_op) + ": " : std::string()) + "HIP error: " + hipGetErrorString(e) + " at " + where);
    return e == hipErrorOutOfMemory ? PA_ENOMEM : PA_EDEVICE;
}
}  // namespace pa

using pa::set_error;

#define PA_CHECK(cond, code, msg) \
    do {                          \
        if (!(cond)) {            \
            set_error(msg);       \
            return code;          \
        }                         \
    } while (0)

namespace {

hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Every build and every reduce gives its index a value no other has had: a
// pa_coverage holds the one it was made under (pa_coverage_*: PA_EINVAL after).
uint64_t next_epoch() {
    static std::atomic<uint64_t> e{0};
    return ++e;
}

pa_status to_dev_params(const pa_params *p, uint32_t n_genomes, pa::DevParams *out) {
    PA_CHECK(p != nullptr, PA_EINVAL, "params must not be NULL");
    PA_CHECK(p->m >= 0, PA_EINVAL, "m must be bigger than or equal to 0");
    PA_CHECK((p->flags & ~7u) == 0, PA_EINVAL, "unknown flag bits in pa_params.flags");
    out->m = (int32_t)clampi(p->m, 0, 1 << 30);
    out->p = (int32_t)clampi(p->p, -1, 1 << 30);
    out->mrq = (int32_t)clampi(p->min_read_quality, 0, 256);
    out->mkq = (int32_t)clampi(p->min_kmer_quality, 0, 256);
    out->mg = (int32_t)clampi(p->max_genomes, -1, (int64_t)n_genomes);
    out->flags = p->flags;
    return PA_OK;
}

// An index a call may use: not NULL, not emptied by a failed reduce.
pa_status check_index(const pa_index *idx) {
    PA_CHECK(idx != nullptr, PA_EINVAL, "NULL argument");
    PA_CHECK(!idx->released, PA_EINVAL, "the index was released by a failed pa_index_reduce: it may only be freed");
    return PA_OK;
}

// A result made for this index, on its device.
pa_status check_result(const pa_index *idx, const pa_result *acc) {
    PA_CHECK(acc->n_genomes == idx->n_genomes, PA_EINVAL, "result was created for a different index");
    PA_CHECK(acc->device == idx->device, PA_EINVAL, "index and result must live on the same device");
    return PA_OK;
}

// ... and a batch of reads on its device.
pa_status check_batch(const pa_index *idx, const pa_reads *reads) {
    PA_CHECK(reads != nullptr, PA_EINVAL, "NULL argument");  // (before the index's state, as ever)
    PA_TRY(check_index(idx));
    PA_CHECK(reads->device == idx->device, PA_EINVAL, "index and reads must live on the same device");
    return PA_OK;
}

// The accumulator of `type` (not NULL) was made for this build of this index.
pa_status check_acc(const pa::AccBase *acc, const pa_index *idx, const char *type) {
    PA_CHECK(pa::acc_matches(*acc, idx), PA_EINVAL,
             std::string("the ") + type + " was made for another index, or for this one before a pa_index_reduce");
    return PA_OK;
}

// A selection of pa_reads_select / pa_extract_fastq_file (not NULL).
pa_status check_extract_spec(const pa_extract_spec *spec) {
    PA_CHECK(pa::extract_mask_ok(spec->type_mask), PA_EINVAL,
             "type_mask must hold at least one of the four type bits and no other");
    PA_CHECK((spec->flags & ~PA_EXTRACT_INVERT) == 0, PA_EINVAL, "unknown flag bits in pa_extract_spec.flags");
    return PA_OK;
}

// The trim of a pa_*_fastq_*_ex call (opts nullable): the spec checked, as the
// streams take it; the windows' statistics summed here and added to the
// caller's only when the call succeeds (a refused late window leaves them alone).
struct StreamTrimCall {
    pa::TrimSpec spec{};
    pa_trim_stats got{};
    pa::StreamTrim trim;
    pa_trim_stats *dst = nullptr;
    pa_status open(const pa_fastq_opts *opts) {
        if (!opts || !opts->trim) return PA_OK;
        PA_TRY(pa::trim_spec_check(opts->trim, &spec));
        trim.spec = &spec;
        trim.stats = &got;
        dst = opts->trim_stats;
        return PA_OK;
    }
    pa_status finish(pa_status rc) {
        if (rc == PA_OK && dst) pa::trim_stats_add(dst, got);
        return rc;
    }
};

// The index's device current and its align-side view made.
pa_status prepare_pass(const pa_index *idx, void *stream) {
    PA_HIP(hipSetDevice(idx->device));
    return pa::index_prepare(const_cast<pa_index *>(idx), as_stream(stream));
}

// What every per-batch entry point starts with, in this order: the handles,
// the parameters, the device, the index's align-side view.
pa_status begin_align(const pa_index *idx, const pa_reads *reads, const pa_params *params, void *stream,
                      pa::DevParams *dp) {
    PA_TRY(check_batch(idx, reads));
    PA_TRY(to_dev_params(params, idx->n_genomes, dp));
    return prepare_pass(idx, stream);
}

}  // namespace

extern "C" {

const char *pa_last_error(void) { return pa::g_err.c_str(); }

// PA_SOURCE_HASH: SHA-256 of csrc/*, include/pa.h and the compile flags, put on
// this file's command line by build_native.py, so a test or a bench line can
// tie the loaded binary to the checkout it came from.
#ifndef PA_SOURCE_HASH
#define PA_SOURCE_HASH "unknown"
#endif
const char *pa_version(void) { return "libpa 0.2 (gfx950) src=" PA_SOURCE_HASH; }

namespace {
struct RuntimeStarter {  // joined at exit, before the HIP runtime's own teardown (it was loaded first)
    std::thread th;
    bool started = false;
    ~RuntimeStarter() {
        if (th.joinable()) th.join();
    }
};
RuntimeStarter g_runtime_starter;
}  // namespace

pa_status pa_runtime_start(int32_t device) {
    if (g_runtime_starter.started) return PA_OK;
    g_runtime_starter.started = true;
    g_runtime_starter.th = std::thread([device] {
        const auto t0 = std::chrono::steady_clock::now();
        // (PA_RUNTIME_WARM=0: the context only, A/B)
        if (hipSetDevice(device) == hipSuccess && hipFree(nullptr) == hipSuccess &&
            !pa::env_is("PA_RUNTIME_WARM", '0')) {
            pa::warm_index(nullptr);  // the code objects too, not at the first real launch
            pa::warm_align(nullptr);
            pa::warm_fastq(nullptr);
            pa::warm_dump(nullptr);
            hipDeviceSynchronize();
        }
        if (pa::env_is("PA_CLI_TIMING", '1'))
            fprintf(stderr, "[pa_runtime] HIP runtime started in %.1f ms\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    });
    return PA_OK;
}

pa_status pa_runtime_wait(void) {
    if (g_runtime_starter.th.joinable()) g_runtime_starter.th.join();
    return PA_OK;
}

pa_status pa_device_count(int32_t *n) {
    PA_CHECK(n != nullptr, PA_EINVAL, "n must not be NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        set_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
        return PA_EDEVICE;
    }
    *n = c;
    return PA_OK;
}

pa_status pa_index_build(int32_t device, const char *genomes, const uint64_t *genome_off, uint32_t n_genomes,
                         int64_t k, void *stream, pa_index **out) {
    return pa_index_build_ex(device, genomes, genome_off, n_genomes, k, 0u, stream, out);
}

pa_status pa_index_build_ex(int32_t device, const char *genomes, const uint64_t *genome_off, uint32_t n_genomes,
                            int64_t k, uint32_t flags, void *stream, pa_index **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "out must not be NULL");
    *out = nullptr;
    PA_CHECK((flags & ~(PA_BUILD_DEFER_TILES | PA_BUILD_COMPACT | PA_BUILD_BOTH_STRANDS)) == 0, PA_EINVAL,
             "unknown build flag bits");
    PA_CHECK(genome_off != nullptr, PA_EINVAL, "genome_off must not be NULL");
    PA_CHECK(k <= PA_MAX_K, PA_EUNSUPPORTED, "k-mer length above PA_MAX_K (255) is not supported");
    PA_CHECK(n_genomes <= PA_MAX_GENOMES, PA_EUNSUPPORTED,
             "more than PA_MAX_GENOMES (2^20 - 1) genomes: the Summary order keys hold a list position in 20 bits");
    for (uint32_t g = 0; g < n_genomes; g++)
        PA_CHECK(genome_off[g + 1] >= genome_off[g], PA_EINVAL, "genome_off must be non-decreasing");
    const uint64_t total = genome_off[n_genomes] - genome_off[0];
    PA_CHECK(total == 0 || genomes != nullptr, PA_EINVAL, "genomes must not be NULL");
    // (FASTA grammar: genome text is uppercase ACGTN, src/constants.py:1-6, src/records.py:225-233 --
    // checked on the device by the build's encode pass, PA_EINVAL with the first bad byte)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device available (libpa.so has no CPU fallback)");
        return PA_EDEVICE;
    }
    PA_CHECK(device >= 0 && device < ndev, PA_EINVAL, "device ordinal out of range");
    PA_HIP(hipSetDevice(device));
    pa_index *idx = new (std::nothrow) pa_index();
    PA_CHECK(idx != nullptr, PA_ENOMEM, "out of host memory");
    idx->device = device;
    idx->compact_table = (flags & PA_BUILD_COMPACT) != 0;
    idx->both_strands = (flags & PA_BUILD_BOTH_STRANDS) != 0;
    pa_status rc = pa::index_build(idx, genomes, genome_off, n_genomes, k, as_stream(stream),
                                   (flags & PA_BUILD_DEFER_TILES) != 0);
    if (rc != PA_OK) {
        pa::index_release(idx);
        delete idx;
        return rc;
    }
    idx->epoch = next_epoch();
    *out = idx;
    return PA_OK;
}

pa_status pa_index_reduce(pa_index *idx, const uint32_t *keep, uint32_t n_keep, uint32_t flags, void *stream) {
    PA_CHECK(n_keep == 0 || keep != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    for (uint32_t i = 0; i < n_keep; i++) {
        PA_CHECK(keep[i] < idx->n_genomes, PA_EINVAL, "genome number out of range");
        PA_CHECK(i == 0 || keep[i] > keep[i - 1], PA_EINVAL, "genome numbers must be ascending");
    }
    PA_CHECK((flags & ~(PA_BUILD_DEFER_TILES | PA_BUILD_COMPACT)) == 0, PA_EINVAL, "unknown build flag bits");
    PA_HIP(hipSetDevice(idx->device));
    idx->compact_table = (flags & PA_BUILD_COMPACT) != 0;
    const pa_status rc = pa::index_reduce(idx, keep, n_keep, as_stream(stream), (flags & PA_BUILD_DEFER_TILES) != 0);
    // (rebuilt or released: the positions view went with the old index, index_release;
    // a failure that left the index unchanged leaves its view and its pa_coverage objects valid)
    if (rc == PA_OK || idx->released) idx->epoch = next_epoch();
    return rc;
}

pa_status pa_index_prepare(pa_index *idx, void *stream) {
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    PA_TRY(pa::index_prepare(idx, as_stream(stream), ~0ull, true));
    PA_HIP(hipStreamSynchronize(as_stream(stream)));
    return PA_OK;
}

pa_status pa_index_prepare_ex(pa_index *idx, uint64_t expected_reads, void *stream) {
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    PA_TRY(pa::index_prepare(idx, as_stream(stream), expected_reads, true));
    PA_HIP(hipStreamSynchronize(as_stream(stream)));
    return PA_OK;
}

void pa_index_free(pa_index *idx) {
    if (!idx) return;
    hipSetDevice(idx->device);
    pa::index_release(idx);
    delete idx;
}

pa_status pa_index_get_info(const pa_index *idx, pa_index_info *out) {
    PA_CHECK(idx && out, PA_EINVAL, "NULL argument");
    std::memset(out, 0, sizeof(*out));
    out->k = (uint32_t)std::max<int64_t>(idx->k, 0);
    out->n_genomes = idx->n_genomes;
    out->key_words = (uint32_t)idx->nw;
    out->slot_bytes = (uint32_t)pa::slot_bytes(idx->nw);
    out->n_kmers = idx->n_kmers;
    out->n_multi_classes = idx->n_multi;
    out->class_genome_entries = idx->class_entries;
    out->table_slots = idx->cap;
    out->table_bytes = idx->cap * (uint64_t)pa::slot_bytes(idx->nw);
    out->total_windows = idx->total_windows;
    out->device_bytes = idx->device_bytes;
    return PA_OK;
}

pa_status pa_index_strands(const pa_index *idx, uint32_t *both) {
    PA_CHECK(idx && both, PA_EINVAL, "NULL argument");
    *both = idx->both_strands ? 1u : 0u;
    return PA_OK;
}

pa_status pa_index_lookup(const pa_index *idx, const char *kmers, uint64_t n, uint32_t kmer_len, int64_t *cls_out,
                          uint32_t *size_out, void *stream) {
    PA_CHECK(cls_out && (n == 0 || kmers), PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    return pa::index_lookup(idx, kmers, n, kmer_len, cls_out, size_out, as_stream(stream));
}

pa_status pa_index_positions(const pa_index *idx, const char *kmers, uint64_t n, uint32_t kmer_len, uint32_t flags,
                             pa_kmer_hit *hits, uint64_t cap, uint64_t *n_hits, void *stream) {
    PA_CHECK(n_hits && (n == 0 || kmers), PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    PA_CHECK((flags & ~PA_POS_REVERSE) == 0, PA_EINVAL, "unknown flag bits");
    PA_CHECK(n < PA_POS_RC_BIT, PA_EINVAL, "too many queries");
    PA_HIP(hipSetDevice(idx->device));
    return pa::index_positions(idx, kmers, n, kmer_len, flags, hits, cap, n_hits, as_stream(stream));
}

pa_status pa_index_class_genomes(const pa_index *idx, int64_t cls, uint32_t *genomes, uint32_t cap, uint32_t *n,
                                 void *stream) {
    PA_CHECK(n != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    PA_CHECK(cls >= 0 && (uint64_t)cls < (uint64_t)idx->n_genomes + idx->class_entries, PA_EINVAL,
             "class id out of range");
    if ((uint64_t)cls < idx->n_genomes) {
        *n = 1;
        if (genomes && cap >= 1) genomes[0] = (uint32_t)cls;
        return PA_OK;
    }
    // multi-genome class: id = G + word offset of its [size, genomes...] record
    PA_HIP(hipSetDevice(idx->device));
    const uint64_t rec = (uint64_t)cls - idx->n_genomes;
    uint32_t size = 0;
    hipStream_t st = as_stream(stream);
    PA_HIP(hipMemcpyAsync(&size, idx->class_genomes + rec, 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    PA_CHECK(rec + 1 + size <= idx->class_entries, PA_EINVAL, "not a class id");
    *n = size;
    if (genomes && cap > 0) {
        PA_HIP(hipMemcpyAsync(genomes, idx->class_genomes + rec + 1, (uint64_t)std::min(cap, size) * 4,
                              hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
    }
    return PA_OK;
}

pa_status pa_index_extsim_stats(const pa_index *idx, const uint32_t *group_of, uint32_t n_groups, uint64_t *total,
                                uint64_t *uniq, uint64_t *inter, void *stream) {
    PA_CHECK(idx && total && uniq && inter && (idx->n_genomes == 0 || group_of), PA_EINVAL, "NULL argument");
    PA_CHECK(!idx->released, PA_EINVAL, "the index was released by a failed pa_index_reduce: it may only be freed");
    for (uint32_t g = 0; g < idx->n_genomes; g++)
        PA_CHECK(group_of[g] < n_groups, PA_EINVAL, "group_of entry out of range");
    PA_HIP(hipSetDevice(idx->device));
    return pa::index_extsim_stats(idx, group_of, n_groups, total, uniq, inter, as_stream(stream));
}

pa_status pa_reads_upload(int32_t device, const uint8_t *seq, const uint8_t *qual, const uint64_t *read_off,
                          uint64_t n_reads, void *stream, pa_reads **out) {
    PA_CHECK(out && read_off, PA_EINVAL, "NULL argument");
    *out = nullptr;
    const uint64_t nb = read_off[n_reads] - read_off[0];
    PA_CHECK(nb == 0 || (seq && qual), PA_EINVAL, "seq/qual must not be NULL");
    uint32_t max_len = 0;
    for (uint64_t i = 0; i < n_reads; i++) {
        PA_CHECK(read_off[i + 1] >= read_off[i], PA_EINVAL, "read_off must be non-decreasing");
        uint64_t l = read_off[i + 1] - read_off[i];
        PA_CHECK(l < (1ull << 31), PA_EUNSUPPORTED, "reads longer than 2^31 bases are not supported");
        max_len = std::max<uint32_t>(max_len, (uint32_t)l);
    }
    PA_HIP(hipSetDevice(device));
    pa::ErrOp op("pa_reads_upload");
    std::unique_ptr<pa_reads, void (*)(pa_reads *)> r(new (std::nothrow) pa_reads(), pa_reads_free);
    PA_CHECK(r != nullptr, PA_ENOMEM, "out of host memory");
    r->device = device;
    r->n = n_reads;
    r->n_bases = nb;
    r->max_len = max_len;
    hipStream_t st = as_stream(stream);
    PA_HIP(pa::dev_malloc(&r->seq, nb + pa::kReadPad));
    PA_HIP(pa::dev_malloc(&r->qual, nb + pa::kReadPad));
    PA_HIP(pa::dev_malloc(&r->off, (n_reads + 1) * 8));
    if (nb) {
        PA_HIP(hipMemcpyAsync(r->seq, seq + read_off[0], nb, hipMemcpyHostToDevice, st));
        PA_HIP(hipMemcpyAsync(r->qual, qual + read_off[0], nb, hipMemcpyHostToDevice, st));
    }
    std::vector<uint64_t> rebased;  // (offsets that do not start at 0)
    if (read_off[0] != 0) {
        rebased.resize(n_reads + 1);
        for (uint64_t i = 0; i <= n_reads; i++) rebased[i] = read_off[i] - read_off[0];
    }
    PA_HIP(hipMemcpyAsync(r->off, rebased.empty() ? read_off : rebased.data(), (n_reads + 1) * 8, hipMemcpyHostToDevice,
                          st));
    PA_HIP(hipStreamSynchronize(st));
    PA_TRY(pa::reads_measure(r.get(), st));
    *out = r.release();
    return PA_OK;
}

pa_status pa_reads_synthesize_mix(const pa_index *idx, uint64_t n_reads, uint32_t read_len, uint64_t first_read,
                                  uint64_t seed, double sub_rate, double rc_rate, double foreign_rate, void *stream,
                                  pa_reads **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    *out = nullptr;
    PA_CHECK(read_len > 0, PA_EINVAL, "read_len must be positive");
    PA_CHECK(rc_rate >= 0 && foreign_rate >= 0 && rc_rate + foreign_rate <= 1, PA_EINVAL,
             "rc_rate and foreign_rate must be >= 0 with a sum <= 1");
    PA_HIP(hipSetDevice(idx->device));
    std::unique_ptr<pa_reads, void (*)(pa_reads *)> r(new (std::nothrow) pa_reads(), pa_reads_free);
    PA_CHECK(r != nullptr, PA_ENOMEM, "out of host memory");
    r->device = idx->device;
    PA_TRY(pa::reads_synthesize(idx, r.get(), n_reads, read_len, first_read, seed, sub_rate, rc_rate, foreign_rate,
                                as_stream(stream)));
    PA_TRY(pa::reads_measure(r.get(), as_stream(stream)));
    *out = r.release();
    return PA_OK;
}

pa_status pa_reads_synthesize(const pa_index *idx, uint64_t n_reads, uint32_t read_len, uint64_t first_read,
                              uint64_t seed, double sub_rate, void *stream, pa_reads **out) {
    return pa_reads_synthesize_mix(idx, n_reads, read_len, first_read, seed, sub_rate, 0.0, 0.0, stream, out);
}

pa_status pa_reads_info(const pa_reads *reads, uint64_t *n_reads, uint64_t *n_bases, uint32_t *max_len) {
    PA_CHECK(reads != nullptr, PA_EINVAL, "NULL argument");
    if (n_reads) *n_reads = reads->n;
    if (n_bases) *n_bases = reads->n_bases;
    if (max_len) *max_len = reads->max_len;
    return PA_OK;
}

pa_status pa_params_effective(const pa_reads *reads, const pa_params *in, pa_params *out, int32_t *q_min,
                              void *stream) {
    PA_CHECK(reads && in && out, PA_EINVAL, "NULL argument");
    pa::DevParams dp, eff;
    PA_TRY(to_dev_params(in, 1u << 20, &dp));
    PA_HIP(hipSetDevice(reads->device));
    PA_TRY(pa::effective_params(reads, dp, eff, as_stream(stream)));
    const pa_params copy = *in;
    *out = copy;
    out->flags = eff.flags;
    if (q_min) *q_min = reads->q_min < 0 ? 255 : reads->q_min;
    return PA_OK;
}

pa_status pa_reads_download(const pa_reads *reads, uint64_t first, uint64_t count, uint8_t *seq, uint8_t *qual,
                            uint64_t *read_off, void *stream) {
    PA_CHECK(reads && read_off, PA_EINVAL, "NULL argument");
    PA_CHECK(first + count <= reads->n, PA_EINVAL, "read range out of bounds");
    PA_HIP(hipSetDevice(reads->device));
    hipStream_t st = as_stream(stream);
    PA_HIP(hipMemcpyAsync(read_off, reads->off + first, (count + 1) * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    const uint64_t b0 = read_off[0], nb = read_off[count] - b0;
    if (nb) {
        if (seq) PA_HIP(hipMemcpyAsync(seq, reads->seq + b0, nb, hipMemcpyDeviceToHost, st));
        if (qual) PA_HIP(hipMemcpyAsync(qual, reads->qual + b0, nb, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
    }
    for (uint64_t i = 0; i <= count; i++) read_off[i] -= b0;
    return PA_OK;
}

pa_status pa_reads_trim(const pa_reads *in, const pa_trim_spec *spec, pa_reads **out, uint32_t *start,
                        uint32_t *end, pa_trim_stats *stats, void *stream) {
    PA_CHECK(in && spec && out, PA_EINVAL, "NULL argument");
    *out = nullptr;
    pa::TrimSpec t;
    PA_TRY(pa::trim_spec_check(spec, &t));
    PA_HIP(hipSetDevice(in->device));
    std::unique_ptr<pa_reads, void (*)(pa_reads *)> r(new (std::nothrow) pa_reads(), pa_reads_free);
    PA_CHECK(r != nullptr, PA_ENOMEM, "out of host memory");
    pa_trim_stats got{};  // (the caller's sums move only when the call succeeds)
    PA_TRY(pa::reads_trim(in, t, r.get(), start, end, &got, as_stream(stream)));
    if (stats) pa::trim_stats_add(stats, got);
    *out = r.release();
    return PA_OK;
}

void pa_reads_free(pa_reads *reads) {
    if (!reads) return;
    hipSetDevice(reads->device);
    pa::dev_free(reads->seq);
    pa::dev_free(reads->qual);
    pa::dev_free(reads->off);
    delete reads;
}

pa_status pa_result_create(const pa_index *idx, pa_result **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    *out = nullptr;
    PA_HIP(hipSetDevice(idx->device));
    pa::ErrOp op("pa_result_create");
    std::unique_ptr<pa_result, void (*)(pa_result *)> r(new (std::nothrow) pa_result(), pa_result_free);
    PA_CHECK(r != nullptr, PA_ENOMEM, "out of host memory");
    r->device = idx->device;
    r->n_genomes = idx->n_genomes;
    const uint64_t G = idx->n_genomes;
    PA_HIP(pa::dev_malloc(&r->sum_block, (6 + 2 * G) * 8));
    PA_HIP(pa::dev_malloc(&r->min_block, std::max<uint64_t>(G, 1) * 8));
    PA_TRY(pa_result_reset(r.get(), nullptr));
    PA_HIP(hipStreamSynchronize(nullptr));
    *out = r.release();
    return PA_OK;
}

pa_status pa_result_reset(pa_result *res, void *stream) {
    PA_CHECK(res != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(res->device));
    return pa::result_reset(res, as_stream(stream));  // async: memset + fill kernel
}

pa_status pa_result_copy_out(const pa_result *res, void *sum_dst, void *min_dst, void *stream) {
    PA_CHECK(res != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(res->device));
    hipStream_t st = as_stream(stream);
    const uint64_t G = res->n_genomes;
    if (sum_dst) PA_HIP(hipMemcpyAsync(sum_dst, res->sum_block, (6 + 2 * G) * 8, hipMemcpyDeviceToDevice, st));
    if (min_dst && G) PA_HIP(hipMemcpyAsync(min_dst, res->min_block, G * 8, hipMemcpyDeviceToDevice, st));
    return PA_OK;
}

pa_status pa_result_copy_in(pa_result *res, const void *sum_src, const void *min_src, void *stream) {
    PA_CHECK(res != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(res->device));
    hipStream_t st = as_stream(stream);
    const uint64_t G = res->n_genomes;
    if (sum_src) PA_HIP(hipMemcpyAsync(res->sum_block, sum_src, (6 + 2 * G) * 8, hipMemcpyDeviceToDevice, st));
    if (min_src && G) PA_HIP(hipMemcpyAsync(res->min_block, min_src, G * 8, hipMemcpyDeviceToDevice, st));
    return PA_OK;
}

pa_status pa_result_load(pa_result *res, const uint64_t *sum_block, const uint64_t *min_block) {
    PA_CHECK(res && sum_block && (res->n_genomes == 0 || min_block), PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(res->device));
    const uint64_t G = res->n_genomes;
    PA_HIP(hipMemcpy(res->sum_block, sum_block, (6 + 2 * G) * 8, hipMemcpyHostToDevice));
    if (G) PA_HIP(hipMemcpy(res->min_block, min_block, G * 8, hipMemcpyHostToDevice));
    return PA_OK;
}

pa_status pa_result_fetch(const pa_result *res, pa_stats *stats, uint64_t *unique_reads, uint64_t *ambiguous_reads,
                          uint64_t *first_key, void *stream) {
    PA_CHECK(res != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(res->device));
    hipStream_t st = as_stream(stream);
    const uint64_t G = res->n_genomes;
    if (stats) PA_HIP(hipMemcpyAsync(stats, res->sum_block, 6 * 8, hipMemcpyDeviceToHost, st));
    if (unique_reads && G) PA_HIP(hipMemcpyAsync(unique_reads, res->sum_block + 6, G * 8, hipMemcpyDeviceToHost, st));
    if (ambiguous_reads && G)
        PA_HIP(hipMemcpyAsync(ambiguous_reads, res->sum_block + 6 + G, G * 8, hipMemcpyDeviceToHost, st));
    if (first_key && G) PA_HIP(hipMemcpyAsync(first_key, res->min_block, G * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

pa_status pa_result_device_view(pa_result *res, uint64_t **sum_block, uint64_t *n_sum, uint64_t **min_block,
                                uint64_t *n_min) {
    PA_CHECK(res != nullptr, PA_EINVAL, "NULL argument");
    if (sum_block) *sum_block = res->sum_block;
    if (n_sum) *n_sum = 6 + 2ull * res->n_genomes;
    if (min_block) *min_block = res->min_block;
    if (n_min) *n_min = res->n_genomes;
    return PA_OK;
}

void pa_result_free(pa_result *res) {
    if (!res) return;
    hipSetDevice(res->device);
    pa::dev_free(res->sum_block);
    pa::dev_free(res->min_block);
    delete res;
}

pa_status pa_align(const pa_index *idx, const pa_reads *reads, const pa_params *params, uint64_t read_index_base,
                   pa_result *acc, void *stream) {
    PA_CHECK(reads && acc, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    PA_CHECK(acc->n_genomes == idx->n_genomes, PA_EINVAL, "result was created for a different index");
    PA_CHECK(reads->device == idx->device && acc->device == idx->device, PA_EINVAL,
             "index, reads and result must live on the same device");
    PA_CHECK(read_index_base + reads->n < (1ull << 44), PA_EUNSUPPORTED, "read index beyond 2^44");
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    PA_HIP(hipSetDevice(idx->device));
    PA_TRY(pa::index_prepare(const_cast<pa_index *>(idx), as_stream(stream)));
    return pa::align(const_cast<pa_index *>(idx), reads, dp, read_index_base, acc, as_stream(stream));
}

pa_status pa_align_fastq_file(const pa_index *idx, const char *path, const pa_params *params,
                              uint64_t read_index_base, pa_result *acc, int32_t threads, uint64_t window_bytes,
                              void *stream, uint64_t *n_reads) {
    return pa_align_fastq_file_ex(idx, path, params, read_index_base, acc, threads, window_bytes, stream, n_reads,
                                  nullptr);
}

pa_status pa_align_fastq_file_ex(const pa_index *idx, const char *path, const pa_params *params,
                                 uint64_t read_index_base, pa_result *acc, int32_t threads, uint64_t window_bytes,
                                 void *stream, uint64_t *n_reads, const pa_fastq_opts *opts) {
    PA_CHECK(path && acc, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    PA_TRY(check_result(idx, acc));
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    StreamTrimCall tc;
    PA_TRY(tc.open(opts));
    PA_HIP(hipSetDevice(idx->device));
    if (n_reads) *n_reads = 0;
    return tc.finish(pa::align_fastq_file(const_cast<pa_index *>(idx), path, dp, read_index_base, acc,
                                          threads > 0 ? threads : 8, window_bytes ? window_bytes : (128ull << 20),
                                          as_stream(stream), n_reads, 0, ~0ull, nullptr, nullptr, -1, nullptr, tc.trim));
}

pa_status pa_align_fastq_range(const pa_index *idx, const char *path, uint64_t offset, uint64_t length,
                               const pa_params *params, uint64_t read_index_base, pa_result *acc, int32_t threads,
                               uint64_t window_bytes, void *stream, uint64_t *n_reads, pa_idset **ids) {
    PA_CHECK(path && acc, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    PA_TRY(check_result(idx, acc));
    PA_CHECK(length > 0, PA_EINVAL, "empty byte range");
    if (ids) *ids = nullptr;
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    PA_HIP(hipSetDevice(idx->device));
    if (n_reads) *n_reads = 0;
    pa_idset *set = nullptr;
    if (ids) {
        set = new (std::nothrow) pa_idset();
        PA_CHECK(set != nullptr, PA_ENOMEM, "out of host memory");
    }
    const pa_status rc = pa::align_fastq_file(const_cast<pa_index *>(idx), path, dp, read_index_base, acc,
                                              threads > 0 ? threads : 8, window_bytes ? window_bytes : (128ull << 20),
                                              as_stream(stream), n_reads, offset, length, set ? &set->h : nullptr);
    if (rc != PA_OK) {
        delete set;
        return rc;
    }
    if (ids) *ids = set;
    return PA_OK;
}

pa_status pa_reads_select(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                          const pa_extract_spec *spec, uint8_t *selected, uint64_t *n_selected, void *stream) {
    PA_CHECK(idx && reads && params && spec && n_selected, PA_EINVAL, "NULL argument");
    PA_TRY(check_extract_spec(spec));
    pa::DevParams dp;
    PA_TRY(begin_align(idx, reads, params, stream, &dp));
    return pa::reads_select(const_cast<pa_index *>(idx), reads, dp, spec, selected, n_selected, as_stream(stream));
}

pa_status pa_extract_fastq_file(const pa_index *idx, const char *path, const pa_params *params,
                                const pa_extract_spec *spec, int32_t out_fd, uint64_t read_index_base,
                                pa_result *acc, int32_t threads, uint64_t window_bytes, void *stream,
                                pa_extract_stats *stats) {
    return pa_extract_fastq_file_ex(idx, path, params, spec, out_fd, read_index_base, acc, threads, window_bytes,
                                    stream, stats, nullptr);
}

pa_status pa_extract_fastq_file_ex(const pa_index *idx, const char *path, const pa_params *params,
                                   const pa_extract_spec *spec, int32_t out_fd, uint64_t read_index_base,
                                   pa_result *acc, int32_t threads, uint64_t window_bytes, void *stream,
                                   pa_extract_stats *stats, const pa_fastq_opts *opts) {
    PA_CHECK(idx && path && params && spec && stats, PA_EINVAL, "NULL argument");
    *stats = pa_extract_stats{};
    PA_TRY(check_index(idx));
    if (acc) PA_TRY(check_result(idx, acc));
    PA_TRY(check_extract_spec(spec));
    PA_CHECK(out_fd >= 0, PA_EINVAL, "bad file descriptor");
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    StreamTrimCall tc;
    PA_TRY(tc.open(opts));
    PA_HIP(hipSetDevice(idx->device));
    return tc.finish(pa::align_fastq_file(const_cast<pa_index *>(idx), path, dp, read_index_base, acc,
                                          threads > 0 ? threads : 8, window_bytes ? window_bytes : (128ull << 20),
                                          as_stream(stream), nullptr, 0, ~0ull, nullptr, spec, out_fd, stats, tc.trim));
}

pa_status pa_idsets_disjoint(const pa_idset *const *sets, uint32_t n_sets, int32_t device, int32_t *disjoint) {
    PA_CHECK(disjoint && (n_sets == 0 || sets), PA_EINVAL, "NULL argument");
    std::vector<const std::vector<uint64_t> *> v;
    for (uint32_t i = 0; i < n_sets; i++) {
        PA_CHECK(sets[i] != nullptr, PA_EINVAL, "NULL id set");
        v.push_back(&sets[i]->h);
    }
    bool d = true;
    PA_TRY(pa::idsets_disjoint(v, device, &d));
    *disjoint = d ? 1 : 0;
    return PA_OK;
}

void pa_idset_free(pa_idset *ids) { delete ids; }

pa_status pa_index_dumpref(const pa_index *idx, const uint8_t *keep, const uint32_t *desc_of, uint32_t n_desc,
                           const char *const *desc_json, int32_t fd, int32_t threads, uint64_t *desc_unique,
                           uint64_t *desc_multi, uint64_t *desc_order, uint32_t *desc_last_genome, uint64_t *n_kmers) {
    PA_CHECK(idx && desc_of && desc_json && desc_unique && desc_multi && desc_order && desc_last_genome, PA_EINVAL,
             "NULL argument");
    PA_CHECK(!idx->released, PA_EINVAL, "the index was released by a failed pa_index_reduce: it may only be freed");
    PA_CHECK(fd >= 0, PA_EINVAL, "bad file descriptor");
    PA_CHECK(!idx->both_strands, PA_EUNSUPPORTED,
             "pa_index_dumpref: a both-strand index holds reverse-complement k-mers the forward k-mer database "
             "does not list; dump from a forward index of the same genomes");
    for (uint32_t d = 0; d < n_desc; d++) PA_CHECK(desc_json[d], PA_EINVAL, "NULL description");
    PA_HIP(hipSetDevice(idx->device));
    return pa::index_dumpref(idx, keep, desc_of, n_desc, desc_json, fd, threads > 0 ? threads : 8, desc_unique,
                             desc_multi, desc_order, desc_last_genome, n_kmers, nullptr);
}

pa_status pa_fastq_prefetch_start(const char *path, int32_t device, int32_t threads, uint64_t window_bytes,
                                  pa_fastq_prefetch **out) {
    PA_CHECK(path && out, PA_EINVAL, "NULL argument");
    *out = nullptr;
    PA_CHECK(device >= 0, PA_EINVAL, "no such device");
    // (no HIP call here: the runtime starts on the prefetch thread, beside the caller's FASTA parse;
    // a bad device is reported by pa_align_fastq_prefetched)
    return pa::fastq_prefetch_start(path, device, threads > 0 ? threads : 8,
                                    window_bytes ? window_bytes : (128ull << 20), out);
}

void pa_fastq_prefetch_free(pa_fastq_prefetch *pf) { pa::fastq_prefetch_free(pf); }

pa_status pa_align_fastq_prefetched(const pa_index *idx, pa_fastq_prefetch *pf, const pa_params *params,
                                    uint64_t read_index_base, pa_result *acc, void *stream, uint64_t *n_reads) {
    return pa_align_fastq_prefetched_ex(idx, pf, params, read_index_base, acc, stream, n_reads, nullptr);
}

pa_status pa_align_fastq_prefetched_ex(const pa_index *idx, pa_fastq_prefetch *pf, const pa_params *params,
                                       uint64_t read_index_base, pa_result *acc, void *stream, uint64_t *n_reads,
                                       const pa_fastq_opts *opts) {
    PA_CHECK(pf && acc, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(idx));
    PA_TRY(check_result(idx, acc));
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    StreamTrimCall tc;
    PA_TRY(tc.open(opts));
    PA_HIP(hipSetDevice(idx->device));
    if (n_reads) *n_reads = 0;
    return tc.finish(pa::align_fastq_prefetched(const_cast<pa_index *>(idx), pf, dp, read_index_base, acc,
                                                as_stream(stream), n_reads, tc.trim));
}

pa_status pa_align_detail(const pa_index *idx, const pa_reads *reads, const pa_params *params, uint8_t *read_type,
                          uint32_t *filtered_kmers, uint32_t *redundant_kmers, uint64_t *list_off, uint32_t *lists,
                          uint64_t list_cap, uint64_t *list_total, void *stream) {
    PA_CHECK(read_type && filtered_kmers && redundant_kmers && list_off, PA_EINVAL, "NULL argument");
    pa::DevParams dp;
    PA_TRY(begin_align(idx, reads, params, stream, &dp));
    return pa::align_detail(const_cast<pa_index *>(idx), reads, dp, read_type, filtered_kmers, redundant_kmers,
                            list_off, lists, list_cap, list_total, as_stream(stream));
}

pa_status pa_align_reads(const pa_index *idx, const pa_reads *reads, const pa_params *params, uint8_t *read_type,
                         uint32_t *filtered_kmers, uint32_t *redundant_kmers, uint64_t *list_off, uint32_t *lists,
                         uint64_t list_cap, uint64_t *list_total, void *stream) {
    PA_CHECK(read_type && list_off && list_total, PA_EINVAL, "NULL argument");
    pa::DevParams dp;
    PA_TRY(begin_align(idx, reads, params, stream, &dp));
    return pa::align_reads(const_cast<pa_index *>(idx), reads, dp, read_type, filtered_kmers, redundant_kmers,
                           list_off, lists, list_cap, list_total, as_stream(stream));
}

pa_status pa_align_pairs(const pa_index *idx, const pa_reads *mates1, const pa_reads *mates2,
                         const pa_params *params, uint64_t pair_index_base, pa_result *acc, uint8_t *pair_type,
                         uint32_t *filtered_kmers, uint32_t *redundant_kmers, uint64_t *list_off, uint32_t *lists,
                         uint64_t list_cap, uint64_t *list_total, uint64_t *exact_pairs, void *stream) {
    PA_CHECK(idx && mates1 && mates2, PA_EINVAL, "NULL argument");
    PA_CHECK(!lists || (pair_type && list_off && list_total), PA_EINVAL,
             "NULL argument (lists need pair_type, list_off and list_total)");
    PA_TRY(check_batch(idx, mates1));
    PA_TRY(check_batch(idx, mates2));
    PA_CHECK(mates1->n == mates2->n, PA_EINVAL,
             "pa_align_pairs: the two batches hold different numbers of reads (mate i of each is one pair)");
    if (acc) PA_TRY(check_result(idx, acc));
    PA_CHECK(mates1->n < 0xFFFFFFFFull, PA_EUNSUPPORTED,
             "pa_align_pairs: a batch holds at most 2^32 - 2 pairs (split it; pair_index_base keeps the order)");
    PA_CHECK(pair_index_base + mates1->n < (1ull << 44), PA_EUNSUPPORTED, "pair index beyond 2^44");
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    if (list_off) list_off[0] = 0;
    if (list_total) *list_total = 0;
    if (exact_pairs) *exact_pairs = 0;
    if (mates1->n == 0) return PA_OK;
    PA_TRY(prepare_pass(idx, stream));
    pa::ErrOp op("pa_align_pairs");
    return pa::align_pairs(const_cast<pa_index *>(idx), mates1, mates2, dp, pair_index_base, acc, pair_type,
                           filtered_kmers, redundant_kmers, list_off, lists, list_cap, list_total, exact_pairs,
                           as_stream(stream));
}

pa_status pa_align_batch(const pa_index *idx, const uint8_t *seq, const uint8_t *qual, const uint64_t *read_off,
                         uint64_t n_reads, uint64_t read_index_base, const pa_params *params, pa_stats *stats,
                         uint64_t *unique_reads, uint64_t *ambiguous_reads, uint64_t *first_key, void *stream) {
    PA_TRY(check_index(idx));
    pa_reads *r = nullptr;
    pa_result *res = nullptr;
    PA_TRY(pa_reads_upload(idx->device, seq, qual, read_off, n_reads, stream, &r));
    pa_status rc = pa_result_create(idx, &res);
    if (rc == PA_OK) rc = pa_align(idx, r, params, read_index_base, res, stream);
    const uint64_t G = idx->n_genomes;
    if (rc == PA_OK) {
        pa_stats s{};
        uint64_t *u = new (std::nothrow) uint64_t[3 * G + 1];
        if (!u) {
            rc = PA_ENOMEM;
        } else {
            rc = pa_result_fetch(res, &s, u, u + G, u + 2 * G, stream);
            if (rc == PA_OK) {
                if (stats) {
                    stats->unique_mapped_reads += s.unique_mapped_reads;
                    stats->ambiguous_mapped_reads += s.ambiguous_mapped_reads;
                    stats->unmapped_reads += s.unmapped_reads;
                    stats->filtered_quality_reads += s.filtered_quality_reads;
                    stats->filtered_quality_kmers += s.filtered_quality_kmers;
                    stats->filtered_hr_kmers += s.filtered_hr_kmers;
                }
                for (uint64_t g = 0; g < G; g++) {
                    if (unique_reads) unique_reads[g] += u[g];
                    if (ambiguous_reads) ambiguous_reads[g] += u[G + g];
                    if (first_key) first_key[g] = std::min(first_key[g], u[2 * G + g]);
                }
            }
            delete[] u;
        }
    }
    pa_result_free(res);
    pa_reads_free(r);
    return rc;
}

// ---- coverage (csrc/pa_cover.hip) ---------------------------------------------------

pa_status pa_index_prepare_coverage(pa_index *idx, void *stream) {
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    PA_TRY(pa::index_prepare_coverage(idx, as_stream(stream)));
    PA_HIP(hipStreamSynchronize(as_stream(stream)));
    return PA_OK;
}

pa_status pa_coverage_create(const pa_index *idx, pa_coverage **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "NULL argument");
    *out = nullptr;
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    return pa::coverage_create(idx, out);
}

pa_status pa_coverage_reset(pa_coverage *cov, void *stream) {
    PA_CHECK(cov != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(cov->device));
    return pa::coverage_reset(cov, as_stream(stream));
}

pa_status pa_coverage_add(const pa_index *idx, const pa_reads *reads, const pa_params *params, pa_coverage *acc,
                          void *stream) {
    PA_CHECK(acc != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_batch(idx, reads));
    PA_TRY(check_acc(acc, idx, "pa_coverage"));
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    PA_CHECK(acc->reads_added + reads->n < (1ull << 32), PA_EUNSUPPORTED,
             "a pa_coverage holds fewer than 2^32 reads (its depths are 32-bit)");
    PA_TRY(prepare_pass(idx, stream));
    return pa::coverage_place(const_cast<pa_index *>(idx), reads, dp, acc, nullptr, nullptr, nullptr, nullptr, 0,
                              nullptr, as_stream(stream));
}

pa_status pa_coverage_summary(const pa_coverage *cov, uint32_t min_coverage, uint64_t *covered_unique,
                              uint64_t *covered_ambiguous, uint64_t *sum_unique, uint64_t *sum_ambiguous,
                              void *stream) {
    PA_CHECK(cov != nullptr, PA_EINVAL, "NULL argument");
    PA_CHECK(min_coverage >= 1, PA_EINVAL, "min_coverage must be at least 1");
    PA_HIP(hipSetDevice(cov->device));
    return pa::coverage_summary(const_cast<pa_coverage *>(cov), min_coverage, covered_unique, covered_ambiguous,
                                sum_unique, sum_ambiguous, as_stream(stream));
}

pa_status pa_coverage_depth(const pa_coverage *cov, uint32_t genome, uint64_t first, uint64_t count,
                            uint32_t *unique_depth, uint32_t *ambiguous_depth, void *stream) {
    PA_CHECK(cov != nullptr, PA_EINVAL, "NULL argument");
    PA_CHECK(genome < cov->n_genomes, PA_EINVAL, "genome number out of range");
    const uint64_t len = cov->h_foff[genome + 1] - cov->h_foff[genome];
    PA_CHECK(first <= len && count <= len - first, PA_EINVAL, "positions past the end of the genome");
    PA_HIP(hipSetDevice(cov->device));
    return pa::coverage_depth(const_cast<pa_coverage *>(cov), genome, first, count, unique_depth, ambiguous_depth,
                              as_stream(stream));
}

void pa_coverage_free(pa_coverage *cov) {
    if (!cov) return;
    hipSetDevice(cov->device);
    pa::coverage_free(cov);
}

pa_status pa_align_placements(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                              uint8_t *read_type, uint64_t *list_off, uint32_t *lists, int64_t *starts,
                              uint64_t list_cap, uint64_t *list_total, void *stream) {
    PA_CHECK(read_type && list_off, PA_EINVAL, "NULL argument");
    pa::DevParams dp;
    PA_TRY(begin_align(idx, reads, params, stream, &dp));
    return pa::coverage_place(const_cast<pa_index *>(idx), reads, dp, nullptr, read_type, list_off, lists, starts,
                              list_cap, list_total, as_stream(stream));
}

// ---- pileup (csrc/pa_pileup.hip) ------------------------------------------------------

pa_status pa_pileup_create(const pa_index *idx, pa_pileup **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "NULL argument");
    *out = nullptr;
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    return pa::pileup_create(idx, out);
}

pa_status pa_pileup_reset(pa_pileup *p, void *stream) {
    PA_CHECK(p != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(p->device));
    return pa::pileup_reset(p, as_stream(stream));
}

pa_status pa_pileup_add(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                        uint32_t min_base_quality, pa_pileup *acc, void *stream) {
    PA_CHECK(acc != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_batch(idx, reads));
    PA_TRY(check_acc(acc, idx, "pa_pileup"));
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    PA_CHECK(acc->reads_added + reads->n < (1ull << 32), PA_EUNSUPPORTED,
             "a pa_pileup holds fewer than 2^32 reads (its counts are 32-bit)");
    PA_TRY(prepare_pass(idx, stream));
    return pa::pileup_add(const_cast<pa_index *>(idx), reads, dp, min_base_quality, acc, as_stream(stream));
}

pa_status pa_pileup_stats_get(const pa_pileup *p, pa_pileup_stats *out, void *stream) {
    PA_CHECK(p && out, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(p->device));
    return pa::pileup_stats(p, out, as_stream(stream));
}

pa_status pa_pileup_counts(const pa_pileup *p, uint32_t genome, uint64_t first, uint64_t count, uint32_t *acgt,
                           void *stream) {
    PA_CHECK(p != nullptr, PA_EINVAL, "NULL argument");
    PA_CHECK(genome < p->n_genomes, PA_EINVAL, "genome number out of range");
    const uint64_t len = p->h_foff[genome + 1] - p->h_foff[genome];
    PA_CHECK(first <= len && count <= len - first, PA_EINVAL, "positions past the end of the genome");
    PA_CHECK(acgt != nullptr || count == 0, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(p->device));
    return pa::pileup_counts(p, genome, first, count, acgt, as_stream(stream));
}

pa_status pa_pileup_variants(const pa_pileup *p, uint32_t min_depth, uint32_t min_alt_count,
                             uint32_t min_alt_permille, pa_variant *out, uint64_t cap, uint64_t *n, void *stream) {
    PA_CHECK(p && n, PA_EINVAL, "NULL argument");
    *n = 0;
    PA_CHECK(min_depth >= 1, PA_EINVAL, "min_depth must be at least 1");
    PA_CHECK(min_alt_count >= 1, PA_EINVAL, "min_alt_count must be at least 1");
    PA_CHECK(min_alt_permille <= 1000, PA_EINVAL, "min_alt_permille must be at most 1000");
    PA_HIP(hipSetDevice(p->device));
    return pa::pileup_variants(p, min_depth, min_alt_count, min_alt_permille, out, out ? cap : 0, n,
                               as_stream(stream));
}

void pa_pileup_free(pa_pileup *p) {
    if (!p) return;
    hipSetDevice(p->device);
    pa::pileup_free(p);
}

// ---- abundance (csrc/pa_abund.hip) ------------------------------------------------------

pa_status pa_abundance_create(const pa_index *idx, pa_abundance **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "NULL argument");
    *out = nullptr;
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    return pa::abundance_create(idx, out);
}

pa_status pa_abundance_reset(pa_abundance *a, void *stream) {
    PA_CHECK(a != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(a->device));
    return pa::abundance_reset(a, as_stream(stream));
}

pa_status pa_abundance_add(const pa_index *idx, const pa_reads *reads, const pa_params *params, pa_abundance *acc,
                           void *stream) {
    PA_CHECK(acc != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_batch(idx, reads));
    PA_TRY(check_acc(acc, idx, "pa_abundance"));
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    PA_TRY(prepare_pass(idx, stream));
    return pa::abundance_add(const_cast<pa_index *>(idx), reads, dp, acc, as_stream(stream));
}

pa_status pa_abundance_info_get(const pa_abundance *a, pa_abundance_info *out, void *stream) {
    PA_CHECK(a && out, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(a->device));
    return pa::abundance_info(a, out, as_stream(stream));
}

pa_status pa_abundance_classes(const pa_abundance *a, uint64_t *class_off, uint32_t *genomes, uint64_t *counts,
                               uint64_t cap_classes, uint64_t cap_entries, uint64_t *n_classes, uint64_t *n_entries,
                               void *stream) {
    PA_CHECK(a && n_classes && n_entries, PA_EINVAL, "NULL argument");
    *n_classes = *n_entries = 0;
    PA_HIP(hipSetDevice(a->device));
    return pa::abundance_classes(a, class_off, genomes, counts, cap_classes, cap_entries, n_classes, n_entries,
                                 as_stream(stream));
}

pa_status pa_abundance_estimate(const pa_abundance *a, uint32_t max_iterations, double tolerance,
                                double *read_fraction, double *abundance, uint32_t *iterations_done,
                                double *last_delta, void *stream) {
    PA_CHECK(a != nullptr, PA_EINVAL, "NULL argument");
    PA_CHECK(max_iterations >= 1 && max_iterations <= 10000, PA_EINVAL, "max_iterations must be 1 to 10000");
    PA_CHECK(tolerance >= 0, PA_EINVAL, "tolerance must be a number that is not negative");  // (false for NaN too)
    PA_HIP(hipSetDevice(a->device));
    return pa::abundance_estimate(a, max_iterations, tolerance, read_fraction, abundance, iterations_done, last_delta,
                                  as_stream(stream));
}

pa_status pa_abundance_bootstrap(const pa_abundance *a, uint32_t replicates, uint64_t seed, uint32_t max_iterations,
                                 double tolerance, uint64_t *counts, double *read_fraction, double *abundance,
                                 uint32_t *iterations, double *last_delta, void *stream) {
    PA_CHECK(a != nullptr, PA_EINVAL, "NULL argument");
    PA_CHECK(replicates >= 1 && replicates <= 10000, PA_EINVAL, "replicates must be 1 to 10000");
    PA_CHECK(max_iterations >= 1 && max_iterations <= 10000, PA_EINVAL, "max_iterations must be 1 to 10000");
    PA_CHECK(tolerance >= 0, PA_EINVAL, "tolerance must be a number that is not negative");  // (false for NaN too)
    PA_HIP(hipSetDevice(a->device));
    return pa::abundance_bootstrap(a, replicates, seed, max_iterations, tolerance, counts, read_fraction, abundance,
                                   iterations, last_delta, as_stream(stream));
}

void pa_abundance_free(pa_abundance *a) {
    if (!a) return;
    hipSetDevice(a->device);
    pa::abundance_free(a);
}

pa_status pa_align_candidates(const pa_index *idx, const pa_reads *reads, const pa_params *params, uint8_t *read_type,
                              uint64_t *set_off, uint32_t *sets, uint64_t cap, uint64_t *total, void *stream) {
    PA_CHECK(read_type && set_off && total, PA_EINVAL, "NULL argument");
    pa::DevParams dp;
    PA_TRY(begin_align(idx, reads, params, stream, &dp));
    return pa::align_candidates(const_cast<pa_index *>(idx), reads, dp, read_type, set_off, sets, cap, total,
                                as_stream(stream));
}

// ---- lineages (csrc/pa_lineage.hip) -------------------------------------------------------

pa_status pa_lineage_create(const pa_index *idx, const uint32_t *parent, uint32_t n_nodes,
                            const uint32_t *genome_node, pa_lineage **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "NULL argument");
    *out = nullptr;
    PA_TRY(check_index(idx));
    PA_CHECK(parent != nullptr && (genome_node != nullptr || idx->n_genomes == 0), PA_EINVAL, "NULL argument");
    PA_CHECK(n_nodes != PA_NO_NODE, PA_EUNSUPPORTED, "a tree holds at most 2^32 - 2 nodes");
    PA_HIP(hipSetDevice(idx->device));
    return pa::lineage_create(idx, parent, n_nodes, genome_node, out);
}

pa_status pa_lineage_reset(pa_lineage *l, void *stream) {
    PA_CHECK(l != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(l->device));
    pa::ErrOp op("pa_lineage_reset");
    return pa::lineage_reset(l, as_stream(stream));
}

pa_status pa_lineage_add(const pa_index *idx, const pa_reads *reads, const pa_params *params, pa_lineage *acc,
                         uint32_t *read_node, void *stream) {
    PA_CHECK(acc != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_batch(idx, reads));
    PA_TRY(check_acc(acc, idx, "pa_lineage"));
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    PA_CHECK(reads->n <= 0xFFFFFFFEull, PA_EUNSUPPORTED, "a batch of a pa_lineage holds at most 2^32 - 2 reads");
    PA_TRY(prepare_pass(idx, stream));
    pa::ErrOp op("pa_lineage_add");
    return pa::lineage_add(const_cast<pa_index *>(idx), reads, dp, acc, read_node, as_stream(stream));
}

pa_status pa_lineage_counts(const pa_lineage *l, uint64_t *direct, uint64_t *clade, pa_lineage_info *info,
                            void *stream) {
    PA_CHECK(l != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(l->device));
    pa::ErrOp op("pa_lineage_counts");
    return pa::lineage_counts(l, direct, clade, info, as_stream(stream));
}

pa_status pa_lineage_lca(const pa_lineage *l, const uint64_t *set_off, const uint32_t *sets, uint64_t n_sets,
                         uint32_t *node_out, void *stream) {
    PA_CHECK(l != nullptr, PA_EINVAL, "NULL argument");
    PA_CHECK(n_sets == 0 || (set_off && node_out), PA_EINVAL, "NULL argument");
    PA_CHECK(n_sets <= 0xFFFFFFFEull, PA_EUNSUPPORTED, "pa_lineage_lca takes at most 2^32 - 2 sets a call");
    if (n_sets) {
        PA_CHECK(set_off[0] == 0, PA_EINVAL, "set_off must start at 0");
        for (uint64_t i = 0; i < n_sets; i++)
            PA_CHECK(set_off[i] <= set_off[i + 1], PA_EINVAL, "set_off must not descend");
        PA_CHECK(sets != nullptr || set_off[n_sets] == 0, PA_EINVAL, "NULL argument");
    }
    PA_HIP(hipSetDevice(l->device));
    pa::ErrOp op("pa_lineage_lca");
    return pa::lineage_lca(l, set_off, sets, n_sets, node_out, as_stream(stream));
}

void pa_lineage_free(pa_lineage *l) {
    if (!l) return;
    hipSetDevice(l->device);
    pa::lineage_free(l);
}

// ---- containment (csrc/pa_contain.hip) ------------------------------------------------------

pa_status pa_containment_create(const pa_index *idx, pa_containment **out) {
    PA_CHECK(out != nullptr, PA_EINVAL, "NULL argument");
    *out = nullptr;
    PA_TRY(check_index(idx));
    PA_HIP(hipSetDevice(idx->device));
    return pa::containment_create(idx, out);
}

pa_status pa_containment_reset(pa_containment *c, void *stream) {
    PA_CHECK(c != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(c->device));
    pa::ErrOp op("pa_containment_reset");
    return pa::containment_reset(c, as_stream(stream));
}

// (no prepare_pass: the mark kernel reads the table and the classes, so a deferred index stays deferred)
pa_status pa_containment_add(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                             pa_containment *acc, void *stream) {
    PA_CHECK(acc != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_batch(idx, reads));
    PA_TRY(check_acc(acc, idx, "pa_containment"));
    pa::DevParams dp;
    PA_TRY(to_dev_params(params, idx->n_genomes, &dp));
    PA_HIP(hipSetDevice(idx->device));
    pa::ErrOp op("pa_containment_add");
    return pa::containment_add(idx, reads, dp, acc, as_stream(stream));
}

// An accumulator whose index was reduced or freed since cannot be scanned: the
// table its bits number is gone.  (The index a live accumulator names is kept
// alive by its owner, as for every accumulator.)
pa_status pa_containment_counts(const pa_containment *c, uint64_t *kmers, uint64_t *kmers_seen, uint64_t *specific,
                                uint64_t *specific_seen, uint64_t *hits_specific, pa_containment_info *info,
                                void *stream) {
    PA_CHECK(c != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(c->idx));
    PA_TRY(check_acc(c, c->idx, "pa_containment"));
    PA_HIP(hipSetDevice(c->device));
    pa::ErrOp op("pa_containment_counts");
    return pa::containment_counts(c, kmers, kmers_seen, specific, specific_seen, hits_specific, info,
                                  as_stream(stream));
}

pa_status pa_containment_nodes(const pa_containment *c, const pa_lineage *l, uint64_t *direct_kmers,
                               uint64_t *direct_seen, uint64_t *clade_kmers, uint64_t *clade_seen, void *stream) {
    PA_CHECK(c != nullptr && l != nullptr, PA_EINVAL, "NULL argument");
    PA_TRY(check_index(c->idx));
    PA_TRY(check_acc(c, c->idx, "pa_containment"));
    PA_TRY(check_acc(l, c->idx, "pa_lineage"));
    PA_HIP(hipSetDevice(c->device));
    pa::ErrOp op("pa_containment_nodes");
    return pa::containment_nodes(c, l, direct_kmers, direct_seen, clade_kmers, clade_seen, as_stream(stream));
}

void pa_containment_free(pa_containment *c) {
    if (!c) return;
    hipSetDevice(c->device);
    pa::containment_free(c);
}

pa_status pa_profile_enable(pa_index *idx, int32_t enable) {
    PA_CHECK(idx != nullptr, PA_EINVAL, "NULL argument");
    idx->profile = enable != 0;
    return PA_OK;
}

pa_status pa_profile_read(pa_index *idx, double *main_ms, uint64_t *launches, uint64_t *deferred_reads) {
    PA_CHECK(idx != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(idx->device));
    double ms = 0;
    for (size_t i = 0; i < idx->ev_start.size(); i++) {
        PA_HIP(hipEventSynchronize(idx->ev_stop[i]));
        float t = 0;
        PA_HIP(hipEventElapsedTime(&t, idx->ev_start[i], idx->ev_stop[i]));
        ms += t;
        hipEventDestroy(idx->ev_start[i]);
        hipEventDestroy(idx->ev_stop[i]);
    }
    const uint64_t nl = idx->ev_start.size();
    idx->ev_start.clear();
    idx->ev_stop.clear();
    uint64_t dt = 0;
    PA_HIP(hipDeviceSynchronize());
    PA_HIP(hipMemcpy(&dt, idx->counters + 1, 8, hipMemcpyDeviceToHost));
    PA_HIP(hipMemset(idx->counters + 1, 0, 8));
    if (main_ms) *main_ms = ms;
    if (launches) *launches = nl;
    if (deferred_reads) *deferred_reads = dt;
    return PA_OK;
}

pa_status pa_profile_read_kernels(pa_index *idx, double *ms, uint64_t *launches) {
    PA_CHECK(idx != nullptr && ms != nullptr && launches != nullptr, PA_EINVAL, "NULL argument");
    PA_HIP(hipSetDevice(idx->device));
    for (int i = 0; i < PA_PROF_KERNELS; i++) {
        ms[i] = 0;
        launches[i] = 0;
    }
    pa_status rc = PA_OK;
    for (const auto &e : idx->kev) {
        float t = 0;
        hipError_t he = hipEventSynchronize(e.stop);
        if (he == hipSuccess) he = hipEventElapsedTime(&t, e.start, e.stop);
        if (he != hipSuccess && rc == PA_OK) {
            pa::set_error(std::string("pa_profile_read_kernels: ") + hipGetErrorString(he));
            rc = PA_EDEVICE;
        }
        ms[e.slot] += t;
        launches[e.slot]++;
        hipEventDestroy(e.start);
        hipEventDestroy(e.stop);
    }
    idx->kev.clear();
    return rc;
}

}  // extern "C"
