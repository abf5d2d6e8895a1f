// Internal host-side structures of libpa.so (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pa.h"
#include "pa_home.h"

namespace pa {

// Last error, thread-local; set by the PA_* macros below.
void set_error(const std::string &msg);

// Environment switches (tests and A/B runs), read where and when they are used:
// tests flip them between two calls of one process, so nothing is kept.
inline const char *env(const char *name) { return std::getenv(name); }
inline bool env_is(const char *name, char c) { const char *e = env(name); return e && e[0] == c; }
inline uint64_t env_u64(const char *name, uint64_t unset) { const char *e = env(name); return e ? std::strtoull(e, nullptr, 10) : unset; }
inline int env_int(const char *name, int unset) { const char *e = env(name); return e ? std::atoi(e) : unset; }

// The one HIP-error path: the message holds the operation's name (ErrOp, when
// one is set), HIP's text, file:line and the call; the sticky error is cleared;
// a failed device allocation is PA_ENOMEM, everything else PA_EDEVICE.  Device
// scratch is held by scoped owners (Bufs below), so no cleanup runs here.
pa_status hip_failed(hipError_t e, const char *where);
#define PA_STR2(x) #x
#define PA_STR(x) PA_STR2(x)
#define PA_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return ::pa::hip_failed(e_, __FILE__ ":" PA_STR(__LINE__) " (" #call ")"); \
    } while (0)

// The entry point a thread is in, for the messages of the code below it
// ("pa_pileup_add: HIP error: ..."); nests, the innermost name is used.
struct ErrOp {
    const char *prev;
    explicit ErrOp(const char *name);
    ~ErrOp();
    ErrOp(const ErrOp &) = delete;
    ErrOp &operator=(const ErrOp &) = delete;
};
const char *err_op();  // the name in force ("": none), for messages written by hand

#define PA_TRY(call)                         \
    do {                                     \
        pa_status s_ = (call);               \
        if (s_ != PA_OK) return s_;          \
    } while (0)

// Number of 64-bit words of a packed k-mer key: 2k bits, top word < 64 bits
// so that an all-ones top word can never be a key (empty-slot sentinel).
inline int key_words(int64_t k) { return (int)(k / 32) + 1; }
// Bytes per hash-table slot: key words + {uint32 class, uint32 tile position}.
inline int slot_bytes(int nw) { return 8 * nw + 8; }
// Read buffers are over-allocated so a wave may fetch a whole staging window
// (up to 512 B) past any read start without a bounds check.
constexpr uint64_t kReadPad = 1024;

// Device arguments of the per-read kernels (clamped, see pa_api.cpp).
struct DevParams {
    int32_t m, p;          // m >= 0; p < 0 -> no validation
    int32_t mrq, mkq, mg;  // already clamped to ranges where semantics are unchanged
    uint32_t flags;
};

// Device memory (pa_mem.cpp): large buffers from the library's slab pool,
// small ones straight from hipMalloc.  Every device buffer of libpa.so is
// taken and given back through these; dev_mem_info counts the pool's free
// ranges as free.
hipError_t dev_malloc_raw(void **p, size_t n);
template <typename T>
inline hipError_t dev_malloc(T **p, size_t n) {
    return dev_malloc_raw((void **)p, n);
}
hipError_t dev_free(void *p);
template <typename T>
inline void dev_release(T *&p) {  // freed and forgotten: a second call frees nothing
    (void)dev_free((void *)p);
    p = nullptr;
}
// Like dev_malloc but never gives the pool's idle slabs back to the driver to
// make room (whose reclaim stalls): hipErrorOutOfMemory when no free range of
// the pool and no free device memory can hold n bytes.
hipError_t dev_malloc_try(void **p, size_t n);
size_t dev_pool_largest_free();  // the largest free range of the current device's slabs
hipError_t dev_mem_info(size_t *free_b, size_t *total_b);
size_t dev_trim(int dev);
void dev_pool_stats(int dev, size_t *slab_bytes, size_t *free_bytes);

struct Workspace {  // grow-only device scratch owned by an index
    void *ptr = nullptr;
    size_t bytes = 0;
};

// Device buffers of one call, bound to its stream: every return frees them,
// after one wait for the stream (queued work may still touch them).  The
// ownership rule of the host code: a buffer taken
// during a call belongs to a Bufs until the call succeeds and release() hands
// it to the index or accumulator that keeps it.
struct Bufs {
    hipStream_t st;
    std::vector<void *> p;
    explicit Bufs(hipStream_t s) : st(s) {}
    Bufs(const Bufs &) = delete;
    Bufs &operator=(const Bufs &) = delete;
    ~Bufs() {
        if (p.empty()) return;
        (void)hipStreamSynchronize(st);
        for (size_t i = p.size(); i-- > 0;) dev_free(p[i]);  // newest first
    }
    template <typename T>
    hipError_t get(T **out, uint64_t bytes) {
        *out = nullptr;
        const hipError_t e = dev_malloc(out, bytes < 16 ? 16 : bytes);
        if (e == hipSuccess) p.push_back((void *)*out);
        return e;
    }
    // A buffer taken elsewhere (dev_malloc_try, an optional allocation): the holder's from now on.
    void adopt(void *q) {
        if (q) p.push_back(q);
    }
    // Out of the holder, still allocated: the caller (an index, an accumulator) owns it now.
    template <typename T>
    T *release(T *q) {
        drop((const void *)q);
        return q;
    }
    // A large temporary that must go before the next allocation: freed now
    // (after the stream is done with it; the wait's status is returned), the
    // caller's pointer cleared.
    template <typename T>
    hipError_t free(T *&q) {
        hipError_t e = hipSuccess;
        if (q && drop((const void *)q)) {
            e = hipStreamSynchronize(st);
            dev_free((void *)q);
        }
        q = nullptr;
        return e;
    }

   private:
    bool drop(const void *q) {
        for (size_t i = p.size(); i-- > 0;)
            if (p[i] == q) {
                p.erase(p.begin() + (long)i);
                return true;
            }
        return false;
    }
};

// A rocPRIM call's size query, temporary storage (held by b) and run:
//   PA_HIP(with_temp(b, [&](void *tmp, size_t &bytes) { return rocprim::...(tmp, bytes, ...); }));
template <typename F>
inline hipError_t with_temp(Bufs &b, F &&f) {
    size_t bytes = 0;
    void *tmp = nullptr;
    hipError_t e = f(nullptr, bytes);
    if (e == hipSuccess) e = b.get(&tmp, bytes);
    if (e == hipSuccess) e = f(tmp, bytes);
    return e;
}

// A run-time value as a compile-time constant: f(int_c<N>{}) for the first N
// of the list that equals n, else for the last one; every call returns the
// same type, and a value the list does not hold is not instantiated.
template <int N> using int_c = std::integral_constant<int, N>;
template <int N0, int... Ns, class F>
auto with_int(int n, F &&f) {
    if constexpr (sizeof...(Ns) == 0) return f(int_c<N0>{});
    else return n == N0 ? f(int_c<N0>{}) : with_int<Ns...>(n, f);
}
// ... over the key widths of an index (PA_MAX_K bounds nw at 8)
template <class F>
auto with_nw(int nw, F &&f) {
    return with_int<1, 2, 3, 4, 5, 6, 7, 8>(nw, f);
}

}  // namespace pa

struct pa_index {
    int device = 0;
    int64_t k = 0;
    int nw = 1;
    uint32_t n_genomes = 0;
    // open-addressing table: slots of {uint64 key[nw]; uint32 cls; uint32 tpos}
    void *table = nullptr;
    uint64_t cap = 0;
    pad::HomeCfg home{};               // home-slot function
    uint64_t n_kmers = 0;
    // classes: cls < n_genomes means {cls}; cls >= n_genomes is multi class (cls - n_genomes)
    uint64_t n_multi = 0;
    uint64_t *class_off = nullptr;    // [n_multi]
    uint32_t *class_size = nullptr;   // [n_multi]
    uint32_t *class_genomes = nullptr;
    uint64_t class_entries = 0;
    uint64_t *class_mask = nullptr;     // G <= 64: membership mask per set, indexed like class_genomes
    // genome codes (0-3 ACGT, 4 other) kept for read synthesis
    uint8_t *codes = nullptr;
    uint64_t *goff = nullptr;          // device [n_genomes+1]
    std::vector<uint64_t> h_goff;
    uint64_t total_windows = 0;
    int tpos_local = 0;                // slot.tpos genome-local (references of >= 2^32 bases), else concatenated
    uint64_t distinct_estimate = 0;    // HyperLogLog estimate (+3 %) when the table was sized on it, else 0
    int released = 0;                  // a failed pa_index_reduce emptied it: it may only be freed
    int force_large = 0;               // PA_LAYOUT=large: the layout of a reference too large for the default one
    int compact_table = 0;             // PA_BUILD_COMPACT: 2 slots per genome window (a job of few reads)
    // PA_BUILD_BOTH_STRANDS: genome g is held as the region T(g) = g + N + reverse complement(g)
    // (an empty genome stays empty); codes, goff and h_goff describe those regions, and the
    // forward lengths below give the caller's genome coordinates (positions, read synthesis)
    int both_strands = 0;
    std::vector<uint64_t> h_fwd_len;   // [n_genomes] forward bases of genome g (both_strands only)
    uint64_t *fwd_len = nullptr;       // device copy (both_strands only, else null)
    // genome tiling (single-word keys, < 2^32 genome bases): the genomes as one
    // concatenated 2-bit string plus the class of the k-mer starting at every
    // position (NONE where no indexed window starts); slots point into it (tpos)
    uint64_t tile_n = 0;               // concatenated bases (0: no tiling)
    int tiles_pending = 0;             // 1: the tiles below are still to be made (index_prepare)
    uint32_t *tile_cls = nullptr;      // [tile_n]
    uint64_t *tile_pk = nullptr;       // [tile_n / 32 + 32] MSB-first 2-bit words (padded)
    uint64_t *tile_lw = nullptr;       // [4 (tile_n / 64 + 5)] lane-walk blocks: 2-bit words + flag planes (k_tile_walk)
    uint64_t *tile_big = nullptr;      // [tile_n / 64 + 4] plane "set size > tile_big_mg" (pa_align, cached)
    int64_t tile_big_mg = -1;          // the --max-genomes value tile_big was made for (-1: none)
    void *tile_nb = nullptr;           // [3 tile_n] one-substitution neighbour bits (k_nb_first), optional:
    int nb_spec = 0;                   //   1: 64-bit words, present | specific << 32; 0: 32-bit words, present
    void *tile_nb1 = nullptr;          //   its second piece, words nb_split.. (null: one piece; pa_device.h NbW)
    uint64_t nb_split = ~0ull;
    uint32_t *tile_rcnb = nullptr;     // [3 tile_n] the same for the neighbours' reverse complements (present), optional
    int rcnb_pending = 0;              //   1: left for the first pass that queues enough seedless reads (pa_align.hip)
    int rcnb_checks = 0;               //   passes that looked and found too few
    uint32_t *tile_nbbig = nullptr;    // [3 tile_n] neighbour present with a set > tile_nbbig_mg (pa_align, cached)
    int64_t tile_nbbig_mg = -1;
    uint4 *tile_nbm = nullptr;         // [3 tile_n] {present, specific, set > tile_nbm_mg, 0}: tile_nb and tile_nbbig
    int64_t tile_nbm_mg = -1;          //   interleaved, one 16-B load per mismatch (pa_align, cached; when it fits)
    int nb_skip = 0;                   // (index_prepare) make the tiles without the neighbour bits
    int nb_pending = 0;                // 1: tiles made, neighbour bits not yet (too few reads expected)
    uint64_t reads_seen = 0;           // reads aligned so far (the neighbour bits follow at kNbReadsPerKBase / 1000 per base)
    uint32_t *tile_gblk = nullptr;     // [(tile_n >> 16) + 2] the genome holding position j << 16
    uint64_t *bloom = nullptr;         // [2^bloom_lg] Bloom filter of the table's keys (k_bloom_build), optional
    uint32_t *mm_bits = nullptr;       // [2^mm_lg / 32] minimizer presence bitmap (k_mm_build), optional
    uint32_t mm_lg = 0;
    uint64_t *tile_rcp = nullptr;      // [tile_n / 64 + 5] bit t: the reverse complement of the k-mer at t may be
                                       //   a key (present, or no indexed window at t) -- k_tile_rcp, optional
    uint32_t bloom_lg = 0;
    uint64_t device_bytes = 0;
    // positions view (pa_cover.hip), optional: made by the first coverage / placement call or by
    // pa_index_prepare_coverage, released with the index.  cov_first holds, k-mer after k-mer, the
    // first occurrence (concatenated region position) of the k-mer in each genome of its set, genomes
    // ascending -- the order of its class record; cov_head[slot] is the k-mer's first entry
    uint32_t *cov_head = nullptr;      // [cap] (NONE at empty slots)
    uint32_t *cov_first = nullptr;     // [cov_pairs]
    uint64_t cov_pairs = 0;            // (k-mer, genome) pairs
    uint64_t cov_bytes = 0;            // its share of device_bytes
    int cov_ready = 0;
    uint64_t epoch = 0;                // a new value at every build and reduce (pa_coverage checks it)
    // align scratch
    pa::Workspace ws;
    uint32_t *queue = nullptr;         // read indices deferred to the exact kernel
    uint32_t *queue_hard = nullptr;    // read indices the lane kernel leaves to the wave kernel
    uint32_t *queue_na = nullptr;      // read indices the lane kernel found no seed for (k_align_lane_rc / _na)
    uint32_t *queue_na2 = nullptr;     // those tested window by window (k_align_lane_na)
    uint64_t *queue_na_keys = nullptr; // [2 per queue_na entry] their outer seeds' reverse complements (k_rc_seeds)
    uint32_t *queue_rc = nullptr;      // reads with a reverse-complement seed (k_align_lane_rc)
    uint64_t *queue_rc_anc = nullptr;  //   its first occurrence | seed << 63
    uint4 *qmask = nullptr;            // per read: windows failing --min-kmer-quality (k_quality_masks)
    uint8_t *qdrop = nullptr;          // per read: fails --min-read-quality
    uint64_t qmask_cap = 0;
    unsigned long long *na_count = nullptr;
    uint32_t *seg_cnt = nullptr;       // [kSegMaxWaves] the lane kernel's per-wave queue segments (pa_align.hip)
    uint64_t queue_cap = 0;            // entries of every queue (the reads of a batch + kSegSlack)
    uint64_t *counters = nullptr;      // [0] queue length, [1] deferred total, [2] error flags, [3] hard reads,
                                       // [4..39] PA_STATS counters
    // profiling
    bool profile = false;
    std::vector<hipEvent_t> ev_start, ev_stop;
    struct KernelEvents {
        int slot;  // PA_PROF_* (include/pa.h)
        hipEvent_t start, stop;
    };
    std::vector<KernelEvents> kev;     // one pair per kernel launch of the align pass
    double prof_ms = 0;
    uint64_t prof_launches = 0;
};

namespace pa {
// The one list of an index's align-side view: every buffer made by
// index_prepare, the neighbour-bit builds and the align pass's cached planes,
// and the state that describes them.  Afterwards the index is one without a
// tiling (the exact kernel serves it); a second call frees nothing.
inline void release_align_view(pa_index *idx) {
    dev_release(idx->tile_cls);
    dev_release(idx->tile_pk);
    dev_release(idx->tile_lw);
    dev_release(idx->tile_gblk);
    dev_release(idx->tile_nb);
    dev_release(idx->tile_nb1);
    dev_release(idx->tile_rcnb);
    dev_release(idx->bloom);
    dev_release(idx->mm_bits);
    dev_release(idx->tile_rcp);
    dev_release(idx->tile_big);
    dev_release(idx->tile_nbbig);
    dev_release(idx->tile_nbm);
    idx->tile_n = 0;
    idx->nb_split = ~0ull;
    idx->nb_spec = idx->nb_pending = idx->rcnb_pending = idx->rcnb_checks = 0;
    idx->bloom_lg = idx->mm_lg = 0;
    idx->tile_big_mg = idx->tile_nbbig_mg = idx->tile_nbm_mg = -1;
}
}  // namespace pa

struct pa_reads {
    int device = 0;
    uint64_t n = 0;
    uint64_t n_bases = 0;
    uint32_t max_len = 0;
    uint8_t *seq = nullptr;
    uint8_t *qual = nullptr;
    uint64_t *off = nullptr;  // [n+1]
    // (pa_align) the smallest quality byte and read length, once measured
    // (-1: not yet): quality thresholds no read can fail are then not applied
    int32_t q_min = -1;
    int64_t len_min = -1;
};

struct pa_idset {  // id hashes of a FASTQ byte range (pa_align_fastq_range)
    std::vector<uint64_t> h;
};

namespace pa {
// What every accumulator of one index starts with.
struct AccBase {
    int device = 0;
    const pa_index *idx = nullptr;     // the index it was made for, at
    uint64_t epoch = 0;                //   this build of it
    uint32_t n_genomes = 0;
};
inline void acc_bind(AccBase &a, const pa_index *idx) {
    a.device = idx->device, a.idx = idx, a.epoch = idx->epoch, a.n_genomes = idx->n_genomes;
}
// false: made for another index, or for this one before a reduce
inline bool acc_matches(const AccBase &a, const pa_index *idx) { return a.idx == idx && a.epoch == idx->epoch; }
// The caller's genome coordinates: the forward bases of every genome [G], and the bases before it [G + 1].
inline std::vector<uint64_t> forward_lengths(const pa_index *idx) {
    std::vector<uint64_t> len(idx->n_genomes);
    for (uint32_t g = 0; g < idx->n_genomes; g++)
        len[g] = idx->both_strands ? idx->h_fwd_len[g] : idx->h_goff[g + 1] - idx->h_goff[g];
    return len;
}
inline std::vector<uint64_t> forward_offsets(const pa_index *idx) {
    std::vector<uint64_t> off(idx->n_genomes + 1, 0);
    const std::vector<uint64_t> len = forward_lengths(idx);
    for (uint32_t g = 0; g < idx->n_genomes; g++) off[g + 1] = off[g] + len[g];
    return off;
}
}  // namespace pa

// Depth accumulator of one index (pa_cover.hip): difference arrays in forward
// genome coordinates, |g| + 1 entries per genome and category (genome g's at
// foff[g] + g), the ambiguous category after the unique one.
struct pa_coverage : pa::AccBase {
    std::vector<uint64_t> h_foff;      // [G+1] forward bases before genome g
    uint64_t *foff = nullptr;          // device copy
    uint64_t entries = 0;              // per category: forward bases + G
    uint32_t *diff = nullptr;          // [2 entries]
    uint32_t *depth = nullptr;         // [2 entries] the scanned accumulator, made on demand
    int depth_valid = 0;
    uint64_t reads_added = 0;
};

// Base-count accumulator of one index (pa_pileup.hip): four uint32 counts (A, C,
// G, T) per forward genome base, position x of genome g at 4 (foff[g] + x).
struct pa_pileup : pa::AccBase {
    int both = 0;
    std::vector<uint64_t> h_foff;      // [G+1] forward bases before genome g
    uint64_t *foff = nullptr;          // device copy
    uint32_t *counts = nullptr;        // [4 h_foff[G]]
    uint8_t *ref = nullptr;            // [h_foff[G]] the forward text's codes (its own copy: the calls outlive a reduce)
    unsigned long long *stats = nullptr;  // [3] reads piled, reads skipped, bases counted
    uint64_t reads_added = 0;
};

// Abundance accumulator of one index (pa_abund.hip): the reads' compatibility
// classes.  The unique reads are counted per genome on the device; the classes
// of the ambiguous reads, a few thousand at most, are merged on the host batch
// after batch, keyed by their ascending genome list (the reported order).
struct pa_abundance : pa::AccBase {
    std::vector<double> h_len;         // [G] L_g = |g| - k + 1 (forward windows)
    unsigned long long *counts = nullptr;  // device [4 + G]: reads unique, ambiguous, unmapped, dropped; unique reads of g
    std::map<std::vector<uint32_t>, uint64_t> classes;  // C -> n_C of the ambiguous reads
};

// Lineage accumulator of one index (pa_lineage.hip): the caller's tree
// renumbered in depth-first preorder (pa_tree.h) and the reads counted per
// node.  The device tables are indexed by preorder number; the counts and
// everything reported are in the caller's node numbers.
struct pa_lineage : pa::AccBase {
    uint32_t n_nodes = 0;
    std::vector<uint32_t> h_parent;    // [n_nodes] the caller's parent array (the clade sums climb it)
    std::vector<uint32_t> h_gpre;      // [G] preorder number of genome g's node (the host copy of gpre)
    uint32_t *parent = nullptr;        // device [n_nodes] preorder number of the parent
    uint32_t *last = nullptr;          // device [n_nodes] the largest preorder number of the subtree
    uint32_t *node_of = nullptr;       // device [n_nodes] preorder number -> the caller's node
    uint32_t *gpre = nullptr;          // device [G]
    unsigned long long *direct = nullptr;  // device [n_nodes] reads with node(r) == v, the caller's v
    unsigned long long *counts = nullptr;  // device [4 + G] as pa_abundance's (candidates_device fills it)
};

// Containment accumulator of one index (pa_contain.hip): one bit per table
// slot, set when a retained window of a read found that k-mer.
struct pa_containment : pa::AccBase {
    uint32_t *bits = nullptr;              // device [cap / 32, rounded up] bit `slot`
    uint64_t bits_bytes = 0;
    unsigned long long *hits = nullptr;    // device [G] retained windows whose set is {g}
    unsigned long long *counters = nullptr;  // device [8]: pa_containment_info's seven, the atomic ORs issued
};

struct pa_result {
    int device = 0;
    uint32_t n_genomes = 0;
    uint64_t *sum_block = nullptr;  // [6 + 2G]
    uint64_t *min_block = nullptr;  // [G]
};

namespace pa {
pa_status index_build(pa_index *idx, const char *genomes, const uint64_t *goff, uint32_t n, int64_t k,
                      hipStream_t st, bool defer_tiles, uint8_t *dev_codes = nullptr);
pa_status index_reduce(pa_index *idx, const uint32_t *sel, uint32_t n, hipStream_t st, bool defer_tiles);
// The tiles of a deferred build (no-op otherwise).  reads_hint: the reads the
// caller expects to align with this index; below kNbReadsPerKBase / 1000 per genome
// base the neighbour bits are left for later (index_note_reads makes them once
// the reads aligned pass that point): they cost ~0.5 ns per base and save
// ~0.25 ns per read on C2 (3.43 vs 1.87 G reads/s; build 0.36 vs 0.24 s).
constexpr uint64_t kNbReadsPerKBase = PA_NB_READS_PER_KBASE;
// reads past the neighbour bits' break-even for an index of `bases` genome
// bases and keys of nw words (two- and three-word keys' bits cost more to make)
inline bool nb_repaid(uint64_t reads, uint64_t bases, int nw = 1) {
    const uint64_t per_k = nw >= 3 ? PA_NB_READS_PER_KBASE_3W : nw == 2 ? PA_NB_READS_PER_KBASE_2W : kNbReadsPerKBase;
    return reads >= (bases * per_k + 999) / 1000;
}
// bases of the region that holds a genome of `len` bases in a both-strand index
inline uint64_t strand_region(uint64_t len) { return len ? 2 * len + 1 : 0; }
// complete: also make neighbour bits left pending, when reads_hint (the reads
// still to come; ~0: unknown) passes the break-even (pa_index_prepare[_ex]).
pa_status index_prepare(pa_index *idx, hipStream_t st, uint64_t reads_hint = ~0ull, bool complete = false);
pa_status index_note_reads(pa_index *idx, uint64_t n, hipStream_t st);
pa_status index_build_rcnb(pa_index *idx, hipStream_t st);  // the pending reverse-complement neighbour bits, now
pa_status index_lookup(const pa_index *idx, const char *kmers, uint64_t n, uint32_t kmer_len, int64_t *cls_out,
                       uint32_t *size_out, hipStream_t st);
pa_status index_positions(const pa_index *idx, const char *kmers, uint64_t n, uint32_t kmer_len, uint32_t flags,
                          pa_kmer_hit *hits, uint64_t cap, uint64_t *n_hits, hipStream_t st);
pa_status index_extsim_stats(const pa_index *idx, const uint32_t *group_of, uint32_t n_groups, uint64_t *total,
                             uint64_t *uniq, uint64_t *inter, hipStream_t st);
pa_status reads_synthesize(const pa_index *idx, pa_reads *r, uint64_t n, uint32_t len, uint64_t first,
                           uint64_t seed, double sub_rate, double rc_rate, double foreign_rate, hipStream_t st);
pa_status align(pa_index *idx, const pa_reads *r, const DevParams &p, uint64_t base, pa_result *acc,
                hipStream_t st);
pa_status align_detail(pa_index *idx, const pa_reads *r, const DevParams &p, uint8_t *type, uint32_t *qf,
                       uint32_t *hr, uint64_t *list_off, uint32_t *lists, uint64_t list_cap, uint64_t *list_total,
                       hipStream_t st);
// The detail pass with everything left on the device (pa_cover.hip): without
// d_lists the per-read type, filter counts and list length; with d_off (n + 1
// offsets) and d_lists the lists themselves.
pa_status detail_pass_device(pa_index *idx, const pa_reads *r, const DevParams &p, uint8_t *d_type, uint32_t *d_qf,
                             uint32_t *d_hr, uint32_t *d_len, const uint64_t *d_off, uint32_t *d_lists,
                             hipStream_t st);
// The assign pass (pa_assign.hip): pa_align_detail's per-read outputs, made by
// the lane kernels for the reads they settle (one store per read at their
// commit) and by the exact kernel, in detail mode over the lane chain's queue,
// for the rest.  Device arrays per read of the batch:
struct AssignBufs {
    uint8_t *type;      // PA_*; kAssignUnset until a kernel settles the read
    uint32_t *qf, *hr;  // filtered_kmers, redundant_kmers
    uint32_t *len;      // list length
    uint32_t *g;        // a lane-settled unique read's genome (kAssignNoGenome: none, or the exact kernel's read)
    void *scratch;      // (6 + 3 G) * 8 bytes: the lane kernels' counters go here, never to a caller's result
    bool lane;          // false: every read to the exact kernel (PA_ASSIGN=0)
};
constexpr uint8_t kAssignUnset = 0xFF;
constexpr uint32_t kAssignNoGenome = 0xFFFFFFFFu;
// the two halves in pa_align.hip (the kernels' file): types, counts and list lengths; then the exact kernel's lists
pa_status assign_classify(pa_index *idx, const pa_reads *r, const DevParams &p, const AssignBufs &as, bool *queued,
                          hipStream_t st);
pa_status assign_lists(pa_index *idx, const pa_reads *r, const DevParams &p, const AssignBufs &as, bool queued,
                       const uint64_t *d_off, uint32_t *d_lists, hipStream_t st);
// The whole pass with everything left on the device (detail_pass_device's
// sibling): type, qf, hr, len [n], off [n + 1] and total always; lists [total]
// when total <= list_cap (else null: the caller reports PA_EINVAL or only
// wanted the total).  Every read covered, or PA_EINTERNAL.  The buffers belong
// to the caller's Bufs b: they live as long as it does.
struct AssignDev {
    uint8_t *type = nullptr;
    uint32_t *qf = nullptr, *hr = nullptr, *len = nullptr, *lists = nullptr;
    uint64_t *off = nullptr;
    uint64_t total = 0;
};
pa_status assign_pass_device(pa_index *idx, const pa_reads *r, const DevParams &p, uint64_t list_cap, AssignDev &out,
                             Bufs &b, hipStream_t st);
pa_status align_reads(pa_index *idx, const pa_reads *r, const DevParams &p, uint8_t *type, uint32_t *qf, uint32_t *hr,
                      uint64_t *list_off, uint32_t *lists, uint64_t list_cap, uint64_t *list_total, hipStream_t st);
// coverage (pa_cover.hip)
pa_status index_prepare_coverage(pa_index *idx, hipStream_t st);
void index_release_coverage(pa_index *idx);
pa_status coverage_create(const pa_index *idx, pa_coverage **out);
pa_status coverage_reset(pa_coverage *cov, hipStream_t st);
void coverage_free(pa_coverage *cov);
// classify, place and (acc) accumulate; type / list_off / lists / starts: host outputs, nullable
pa_status coverage_place(pa_index *idx, const pa_reads *r, const DevParams &p, pa_coverage *acc, uint8_t *type,
                         uint64_t *list_off, uint32_t *lists, int64_t *starts, uint64_t list_cap,
                         uint64_t *list_total, hipStream_t st);
pa_status coverage_summary(pa_coverage *cov, uint32_t min_coverage, uint64_t *cov_u, uint64_t *cov_a, uint64_t *sum_u,
                           uint64_t *sum_a, hipStream_t st);
pa_status coverage_depth(pa_coverage *cov, uint32_t genome, uint64_t first, uint64_t count, uint32_t *du,
                         uint32_t *da, hipStream_t st);
// What coverage_place and the pileup pass share (pa_cover.hip): the positions
// view, the assign pass left on the device, k_place's workspace and launch.
// as.lists is null and placed false when nothing is listed or as.total >
// list_cap; else starts / agree (when wanted) hold one value per list entry
// and, with acc, the depths are accumulated.  Held by the caller's Bufs b.
struct PlacedDev {
    AssignDev as;
    int64_t *starts = nullptr;  // [as.total] s(read, genome)
    uint8_t *agree = nullptr;   // [as.total] 1: every voting window named that diagonal
    bool placed = false;
};
pa_status place_device(pa_index *idx, const pa_reads *r, const DevParams &p, pa_coverage *acc,
                       uint64_t list_cap, bool want_starts, bool want_agree, PlacedDev &out, Bufs &b, hipStream_t st);
// pileup (pa_pileup.hip)
pa_status pileup_create(const pa_index *idx, pa_pileup **out);
pa_status pileup_reset(pa_pileup *p, hipStream_t st);
void pileup_free(pa_pileup *p);
pa_status pileup_add(pa_index *idx, const pa_reads *r, const DevParams &p, uint32_t min_base_quality, pa_pileup *acc,
                     hipStream_t st);
pa_status pileup_stats(const pa_pileup *p, pa_pileup_stats *out, hipStream_t st);
pa_status pileup_counts(const pa_pileup *p, uint32_t genome, uint64_t first, uint64_t count, uint32_t *acgt,
                        hipStream_t st);
pa_status pileup_variants(const pa_pileup *p, uint32_t min_depth, uint32_t min_alt_count, uint32_t min_alt_permille,
                          pa_variant *out, uint64_t cap, uint64_t *n, hipStream_t st);
// abundance (pa_abund.hip; the candidate kernel is k_align_exact's sibling in pa_align.hip)
pa_status candidates_pass(pa_index *idx, const pa_reads *r, const DevParams &p, const uint32_t *d_queue,
                          const unsigned long long *d_count, uint64_t n_queued, uint32_t *d_len, const uint64_t *d_off,
                          uint32_t *d_sets, hipStream_t st);
pa_status abundance_create(const pa_index *idx, pa_abundance **out);
pa_status abundance_reset(pa_abundance *a, hipStream_t st);
void abundance_free(pa_abundance *a);
pa_status abundance_add(pa_index *idx, const pa_reads *r, const DevParams &p, pa_abundance *acc, hipStream_t st);
pa_status abundance_info(const pa_abundance *a, pa_abundance_info *out, hipStream_t st);
pa_status abundance_classes(const pa_abundance *a, uint64_t *class_off, uint32_t *genomes, uint64_t *counts,
                            uint64_t cap_classes, uint64_t cap_entries, uint64_t *n_classes, uint64_t *n_entries,
                            hipStream_t st);
pa_status abundance_estimate(const pa_abundance *a, uint32_t max_iterations, double tolerance, double *read_fraction,
                             double *abundance, uint32_t *iterations_done, double *last_delta, hipStream_t st);
pa_status abundance_bootstrap(const pa_abundance *a, uint32_t replicates, uint64_t seed, uint32_t max_iterations,
                              double tolerance, uint64_t *counts, double *read_fraction, double *abundance,
                              uint32_t *iterations, double *last_delta, hipStream_t st);
pa_status align_candidates(pa_index *idx, const pa_reads *r, const DevParams &p, uint8_t *type, uint64_t *set_off,
                           uint32_t *sets, uint64_t cap, uint64_t *total, hipStream_t st);
// The candidate pass left on the device (pa_abund.hip; the abundance and the
// lineage accumulators both start from it).  Held by the caller's Bufs b.
struct CandDev {
    AssignDev as;
    uint32_t *queue = nullptr;   // [n] the ambiguous reads, nq of them
    uint64_t nq = 0;
    uint32_t *len = nullptr;     // [n + 1] set sizes
    uint64_t *off = nullptr;     // [n + 1]
    uint32_t *sets = nullptr;    // [total] (null when total > cap or 0)
    uint64_t total = 0;
};
// counts: an accumulator's [4 + G] (reads unique, ambiguous, unmapped, dropped; unique reads of g),
// or null (a scratch array is used).
pa_status candidates_device(pa_index *idx, const pa_reads *r, const DevParams &p, uint64_t cap,
                            unsigned long long *counts, CandDev &out, Bufs &b, hipStream_t st);
// lineage (pa_lineage.hip)
pa_status lineage_create(const pa_index *idx, const uint32_t *parent, uint32_t n_nodes, const uint32_t *genome_node,
                         pa_lineage **out);
pa_status lineage_reset(pa_lineage *l, hipStream_t st);
void lineage_free(pa_lineage *l);
pa_status lineage_add(pa_index *idx, const pa_reads *r, const DevParams &p, pa_lineage *acc, uint32_t *read_node,
                      hipStream_t st);
pa_status lineage_counts(const pa_lineage *l, uint64_t *direct, uint64_t *clade, pa_lineage_info *info,
                         hipStream_t st);
pa_status lineage_lca(const pa_lineage *l, const uint64_t *set_off, const uint32_t *sets, uint64_t n_sets,
                      uint32_t *node_out, hipStream_t st);
// containment (pa_contain.hip): needs the table and the classes only, never the align-side view
pa_status containment_create(const pa_index *idx, pa_containment **out);
pa_status containment_reset(pa_containment *c, hipStream_t st);
void containment_free(pa_containment *c);
pa_status containment_add(const pa_index *idx, const pa_reads *r, const DevParams &p, pa_containment *acc,
                          hipStream_t st);
pa_status containment_counts(const pa_containment *c, uint64_t *kmers, uint64_t *kmers_seen, uint64_t *specific,
                             uint64_t *specific_seen, uint64_t *hits_specific, pa_containment_info *info,
                             hipStream_t st);
pa_status containment_nodes(const pa_containment *c, const pa_lineage *l, uint64_t *direct_kmers,
                            uint64_t *direct_seen, uint64_t *clade_kmers, uint64_t *clade_seen, hipStream_t st);
// pairs (pa_pair.hip; the pair-exact kernel is k_align_exact's sibling in pa_align.hip)
pa_status pair_exact_pass(pa_index *idx, const pa_reads *m1, const pa_reads *m2, const DevParams &p,
                          const uint32_t *d_queue, const unsigned long long *d_count, uint64_t n_queued,
                          uint8_t *d_type, uint32_t *d_qf, uint32_t *d_hr, uint32_t *d_len, const uint64_t *d_off,
                          uint32_t *d_lists, hipStream_t st);
pa_status align_pairs(pa_index *idx, const pa_reads *m1, const pa_reads *m2, const DevParams &p, uint64_t base,
                      pa_result *acc, uint8_t *type, uint32_t *qf, uint32_t *hr, uint64_t *list_off, uint32_t *lists,
                      uint64_t list_cap, uint64_t *list_total, uint64_t *exact_pairs, hipStream_t st);
pa_status reads_measure(pa_reads *r, hipStream_t st);  // q_min / len_min of a batch (at its creation)
// read trimming (pa_trim.hip)
struct TrimSpec {  // a checked pa_trim_spec as the kernel takes it
    uint32_t flags, q3, q5, alen, min_ov, permille;
    uint64_t a0, a1;  // the adapter's two code bit planes, base j at bit j
};
struct TrimOut {  // what the trimmed batch's pa_reads needs
    uint64_t n_bases = 0;
    uint32_t max_len = 0;
    int64_t len_min = 0;
};
// The one place pa_trim_stats are summed: dst += src.
inline void trim_stats_add(pa_trim_stats *dst, const pa_trim_stats &src) {
    dst->reads += src.reads;
    dst->bases_in += src.bases_in;
    dst->bases_out += src.bases_out;
    dst->reads_trimmed += src.reads_trimmed;
    dst->reads_quality += src.reads_quality;
    dst->bases_quality += src.bases_quality;
    dst->reads_adapter += src.reads_adapter;
    dst->bases_adapter += src.bases_adapter;
    dst->reads_empty += src.reads_empty;
}
constexpr int kTrimCounters = 11;  // pa_trim_stats' nine, the longest and the shortest new read
pa_status trim_spec_check(const pa_trim_spec *spec, TrimSpec *out);
pa_status trim_device(const pa_reads *in, uint64_t in_bases, const TrimSpec &t, uint32_t *d_start, uint32_t *d_end,
                      uint32_t *d_len, uint8_t *o_seq, uint8_t *o_qual, uint64_t *o_off, unsigned long long *d_cnt,
                      Bufs &b, pa_trim_stats *stats, TrimOut *out, hipStream_t st);
pa_status reads_trim(const pa_reads *in, const TrimSpec &t, pa_reads *out, uint32_t *start, uint32_t *end,
                     pa_trim_stats *stats, hipStream_t st);
// a trim of the device-parsed streams (null spec: none)
struct StreamTrim {
    const TrimSpec *spec = nullptr;
    pa_trim_stats *stats = nullptr;
};
// the filters an align of batch r applies: quality thresholds no read can fail dropped
pa_status effective_params(const pa_reads *r, const DevParams &p, DevParams &out, hipStream_t st);
pa_status ensure_workspace(pa_index *idx, size_t bytes);
pa_status reserve_queues(pa_index *idx, uint64_t n);  // align queues for batches of up to n reads
pa_status ensure_qmask(pa_index *idx, uint64_t n);    // quality-filter masks for batches of up to n reads
// offset / length: a byte range of a plain file, cut on record boundaries
// (pa_align_fastq_range); ids_out: the range's id hashes; extract: the selected records
// written to out_fd (pa_extract_fastq_file: acc may then be null)
pa_status align_fastq_file(pa_index *idx, const char *path, const DevParams &prm, uint64_t base, pa_result *acc,
                           int threads, uint64_t window, hipStream_t st, uint64_t *n_reads, uint64_t offset = 0,
                           uint64_t length = ~0ull, std::vector<uint64_t> *ids_out = nullptr,
                           const pa_extract_spec *extract = nullptr, int out_fd = -1,
                           pa_extract_stats *extract_stats = nullptr, StreamTrim trim = StreamTrim{});
// read extraction (pa_extract.hip): the state of one
// pa_extract_fastq_file call -- the selection on the device, the output buffer
// of a window (device and pinned, span + 16 bytes each) and the statistics.
struct Extract {
    uint32_t type_mask = 0, invert = 0;
    uint8_t *keep = nullptr;               // device [n_genomes] genome_keep, or null
    unsigned long long *by_type = nullptr; // device [4] selected records per type, over the file
    uint8_t *d_out = nullptr, *h_out = nullptr;
    uint64_t cap = 0;
    int fd = -1;
    pa_extract_stats *stats = nullptr;
    bool timing = false;                   // PA_STREAM_TIMING=1: the per-window split on stderr
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // ev[5]: the window's start
};
bool extract_mask_ok(uint32_t type_mask);
pa_status extract_open(Extract &x, const pa_index *idx, const pa_extract_spec *spec, int fd, uint64_t span,
                       pa_extract_stats *stats, hipStream_t st);
void extract_close(Extract &x);
pa_status extract_window(Extract &x, pa_index *idx, const pa_reads *r, const DevParams &prm, const uint8_t *D,
                         uint64_t t0, uint64_t lo, uint64_t hi, const uint32_t *nl, hipStream_t st);
pa_status reads_select(pa_index *idx, const pa_reads *r, const DevParams &prm, const pa_extract_spec *spec,
                       uint8_t *selected, uint64_t *n_selected, hipStream_t st);
pa_status idsets_disjoint(const std::vector<const std::vector<uint64_t> *> &sets, int device, bool *disjoint);
pa_status fastq_prefetch_start(const char *path, int device, int threads, uint64_t window, pa_fastq_prefetch **out);
void fastq_prefetch_free(pa_fastq_prefetch *pf);
pa_status align_fastq_prefetched(pa_index *idx, pa_fastq_prefetch *pf, const DevParams &prm, uint64_t base,
                                 pa_result *acc, hipStream_t st, uint64_t *n_reads, StreamTrim trim = StreamTrim{});
pa_status index_dumpref(const pa_index *idx, const uint8_t *keep, const uint32_t *desc_of, uint32_t n_desc,
                        const char *const *desc_json, int fd, int threads, uint64_t *desc_unique, uint64_t *desc_multi,
                        uint64_t *desc_order, uint32_t *desc_last_genome, uint64_t *n_kmers_out, hipStream_t st);
pa_status result_reset(pa_result *res, hipStream_t st);
void index_release(pa_index *idx);
void warm_index(hipStream_t st);  // one empty launch per source file: loads its code object
void warm_align(hipStream_t st);
void warm_fastq(hipStream_t st);
void warm_dump(hipStream_t st);
}  // namespace pa

// Test hook (pa_mem.cpp; tests/test_gpu_alloc_paths.py), not part of the ABI:
// the nth call from now of dev_malloc_raw / dev_malloc_try returns
// hipErrorOutOfMemory without calling HIP (0: off); the calls made so far; the
// buffers handed out and not yet given back.
extern "C" void pa_test_alloc_fail_at(int64_t nth);
extern "C" uint64_t pa_test_alloc_calls(void);
extern "C" uint64_t pa_test_alloc_live(void);
