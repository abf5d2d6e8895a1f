// GPU k-mer index build (KmerReference, src/kmer.py:113-150), lookups, EXTSIM
// statistics (src/kmer.py:152-230) and device-side synthetic reads.
//
// Index layout in HBM
//   table          open addressing, linear probing, `cap` slots of
//                  {uint64 key[NW]; uint32 cls; uint32 tpos} (16 B for k <= 31),
//                  whole 64-B lines.  4 slots per genome window when that fits
//                  a third of the free memory, else 2; a reference too large
//                  for either is sized on a HyperLogLog estimate of its
//                  distinct k-mers, 4 / 2.5 / 2 / 1.43 slots per k-mer
//                  (pa_index_plan.h holds every sizing rule of this file).
//   classes        the genome SET of a k-mer (the keys of kmers[kmer] in the
//                  reference) is a "class": cls < G means the singleton {cls};
//                  cls >= G is a deduplicated multi-genome set stored as the
//                  record class_genomes[cls - G] = [size, ascending genomes...]
//                  (one contiguous read in the align kernels; the size serves
//                  --max-genomes).
//   tiling         (k <= 95, every genome < 2^32 bases) the genomes concatenated
//                  in FASTA order as a 2-bit string `tile_pk` plus `tile_cls[t]`
//                  = class of the k-mer starting at concatenated position t
//                  (NONE if no indexed window starts there: N bases, genome
//                  ends).  A slot's tpos is the first position of its key.  A
//                  read that matches a genome stretch is then resolved by ONE
//                  table probe plus a contiguous read of the tiling (pa_lane.h),
//                  each window still verified base for base against the genome.
//   align view     on top of the tiling, each optional and sized by the free
//                  memory: walk blocks, one-substitution neighbour words, the
//                  Bloom filter of the keys, the minimizer bitmap, the
//                  reverse-complement plane and neighbour words.
//
// Build pipeline (stream-ordered; the host waits where it needs a count)
//   index_build    1. ASCII -> 2-bit codes (4 = anything else, e.g. 'N'); a
//                     both-strand index writes g + N + reverse complement(g).
//                  2. the table's capacity (above), the table.
//   build_nw       3. per genome in FASTA order: insert every N-free window
//                     (atomicCAS claim), count distinct genomes per slot with a
//                     per-slot "last genome" atomicMax (launch order = FASTA
//                     order makes this exact), remember the first genome.
//                  4. singletons get cls = genome; multi slots get a
//                     bump-allocated list (k_build_prep; the host reads the
//                     counts).
//                  5. per genome again: append g to the list of every multi slot
//                     it touches (ascending order for free, from launch order).
//                  6. hash every multi list, dedup lists through a second hash
//                     table that grows on overflow, verify each list against its
//                     class representative element by element (a hash collision
//                     is PA_EINTERNAL, never merged silently), assign class ids
//                     and copy representative lists into class_genomes; then the
//                     slots of a probe run in home order (k_table_order,
//                     PA_TABLE_ORDER).
//   index_prepare  7. the align view, one named step each (tile_* below): at the
//                     end of the build, or deferred (PA_BUILD_DEFER_TILES) to
//                     pa_index_prepare / the first align; the neighbour words may
//                     wait further, for the reads that repay them
//                     (index_note_reads).
// What an index owns is listed once: release_align_view (pa_internal.h) for
// step 7's buffers and state, index_release for the rest.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <memory>
#include <cstdio>
#include <string>
#include <vector>

#include "pa_device.h"
#include "pa_index_plan.h"
#include "pa_internal.h"

using namespace pad;
namespace plan = pa::plan;

namespace {

constexpr int kBlock = 256;
constexpr int kRun = 16;  // windows per thread in the genome scans

using pa::env;
using pa::env_int;
using pa::env_is;
using pa::env_u64;

// Windows per thread of the per-genome build scans (insert, fill, tile
// classes): PA_BUILD_RUN overrides (A/B; read once per process).  Fewer per
// thread = more threads in flight per genome launch (the scans are chains of
// dependent random atomics).
inline int build_run() {
    static const int r = [] {
        const int v = env_int("PA_BUILD_RUN", 0);
        return v > 0 && v <= 256 ? v : kRun;
    }();
    return r;
}

// PA_CLI_TIMING=1: the build's phases on stderr (host wall clock, after a sync)
struct PhaseTimer {
    bool on;
    hipStream_t st;
    std::chrono::steady_clock::time_point t0, t;
    std::string out;
    explicit PhaseTimer(hipStream_t s) : on(env_is("PA_CLI_TIMING", '1')), st(s) {
        t0 = t = std::chrono::steady_clock::now();
    }
    void mark(const char *name) {
        if (!on) return;
        hipStreamSynchronize(st);
        const auto n = std::chrono::steady_clock::now();
        char b[96];
        snprintf(b, sizeof b, "%s%s %.1f", out.empty() ? "" : ", ", name,
                 std::chrono::duration<double, std::milli>(n - t).count());
        out += b;
        t = n;
    }
    ~PhaseTimer() {
        if (on)
            fprintf(stderr, "[pa_build] %s ms; total %.1f ms\n", out.c_str(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};
// The build's timer, for the phases of the functions it calls (tiles,
// neighbour bits, Bloom filters): phase_mark is a no-op outside a timed build.
thread_local PhaseTimer *t_phase = nullptr;
inline void phase_mark(const char *name) {
    if (!t_phase) return;
    t_phase->mark(name);
    // device memory at this point: the driver's free bytes, the pool's slabs and their free part (GiB)
    size_t f = 0, t = 0, sb = 0, sf = 0;
    int dev = 0;
    hipGetDevice(&dev);
    hipMemGetInfo(&f, &t);
    pa::dev_pool_stats(dev, &sb, &sf);
    char b[96];
    snprintf(b, sizeof b, " [driver free %.1f, pool %.1f / free %.1f GiB]", f / 1073741824.0, sb / 1073741824.0,
             sf / 1073741824.0);
    t_phase->out += b;
}
// The phases of one entry point (index_build, index_prepare, the neighbour
// bits made later): those of the timed build that called it, else of a timer
// of its own, printed when the guard goes.
struct TimedPhases {
    std::unique_ptr<PhaseTimer> own;
    PhaseTimer *prev;
    explicit TimedPhases(hipStream_t st) : prev(t_phase) {
        if (t_phase) return;
        own.reset(new PhaseTimer(st));
        t_phase = own->on ? own.get() : nullptr;
    }
    ~TimedPhases() { t_phase = prev; }
    void mark(const char *name) {  // index_build's own phases: the time only
        if (own) own->mark(name);
    }
};

inline unsigned grid_for(uint64_t n, unsigned block = kBlock) {
    uint64_t g = (n + block - 1) / block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, 1u << 30));
}
// ... of the grid-stride scans (tables, tilings): at most 65536 blocks
inline unsigned scan_grid(uint64_t n) { return std::min(grid_for(n), 65536u); }

// ASCII -> 2-bit codes (4: N); *bad = the first byte outside A C G T N (the
// FASTA grammar's genome alphabet), ~0 if none.
__global__ void k_encode(const uint8_t *__restrict__ ascii, uint8_t *__restrict__ codes, uint64_t n,
                         unsigned long long *bad) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long first = ~0ull;
    for (; i < n; i += stride) {
        const uint8_t ch = ascii[i];
        const uint32_t c = base_code(ch);
        codes[i] = (uint8_t)c;
        if (c > 3 && ch != 'N' && first == ~0ull) first = i;
    }
    if (first != ~0ull) atomicMin(bad, first);
}

// 16 bytes starting at any byte address, from three aligned 8-B loads (the
// caller guarantees that the aligned words holding them can be read: the ASCII
// staging buffer is aligned and padded by kExpandPad).
__device__ __forceinline__ void load16_any(const uint8_t *__restrict__ p, uint64_t &lo, uint64_t &hi) {
    const uint64_t *a = (const uint64_t *)((uintptr_t)p & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 7) * 8;
    const uint64_t w0 = a[0], w1 = a[1], w2 = a[2];
    lo = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
    hi = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
}

// The ASCII -> code pass of a both-strand index (PA_BUILD_BOTH_STRANDS): genome
// g's forward text ascii[fgoff[g] .. +L) becomes the region codes[egoff[g] ..
// +2L+1) = forward codes, one N code, the reverse complement's codes (3 - code
// read back to front, N stays N); an empty genome has an empty region.  One
// thread makes kExpandRun output bytes, stored as one 16-B word; where they lie
// in one half of one region their source is one run of text, fetched with
// load16_any (ascending for the forward half, descending for the reverse), else
// byte by byte (region ends, the join).  *bad = the first byte outside A C G T N
// as an offset into the forward text, ~0 if none: every forward byte is encoded
// once by the forward halves, which alone report it.
constexpr int kExpandRun = 16;
constexpr uint64_t kExpandPad = 32;
__global__ __launch_bounds__(256) void k_encode_strands(const uint8_t *__restrict__ ascii,
                                                        const uint64_t *__restrict__ fgoff,
                                                        const uint64_t *__restrict__ egoff, uint32_t G,
                                                        uint8_t *__restrict__ codes, unsigned long long *bad) {
    const uint64_t etotal = egoff[G];
    uint64_t e0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kExpandRun;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * kExpandRun;
    unsigned long long first = ~0ull;
    for (; e0 < etotal; e0 += stride) {
        const uint64_t e1 = min(e0 + (uint64_t)kExpandRun, etotal);
        // region holding e0: the last g with egoff[g] <= e0 that is not empty
        uint32_t lo = 0, hi = G;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (egoff[mid] <= e0)
                lo = mid;
            else
                hi = mid;
        }
        uint32_t g = lo;
        uint64_t rs = egoff[g], re = egoff[g + 1];
        while (re <= e0 && g + 1 < G) rs = re, re = egoff[++g + 1];
        uint64_t fs = fgoff[g], L = fgoff[g + 1] - fs;
        uint8_t out[kExpandRun];
        const bool whole = e1 - e0 == kExpandRun && e1 <= re;
        if (whole && e1 - rs <= L) {  // inside the forward half
            const uint64_t src = fs + (e0 - rs);
            uint64_t w[2];
            load16_any(ascii + src, w[0], w[1]);
#pragma unroll
            for (int i = 0; i < kExpandRun; i++) {
                const uint32_t ch = (uint32_t)(w[i >> 3] >> (8 * (i & 7))) & 0xFFu;
                const uint32_t c = base_code(ch);
                out[i] = (uint8_t)c;
                if (c > 3 && ch != 'N' && first == ~0ull) first = src + i;
            }
        } else if (whole && e0 - rs > L) {  // inside the reverse half: output p <- forward 2L - p
            const uint64_t src = fs + 2 * L - (e1 - 1 - rs);  // the lowest forward byte read
            uint64_t w[2];
            load16_any(ascii + src, w[0], w[1]);
#pragma unroll
            for (int i = 0; i < kExpandRun; i++) {
                const int j = kExpandRun - 1 - i;
                const uint32_t c = base_code((uint32_t)(w[j >> 3] >> (8 * (j & 7))) & 0xFFu);
                out[i] = (uint8_t)(c > 3 ? 4u : 3u - c);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kExpandRun; i++) {
                const uint64_t e = e0 + i;
                out[i] = 4;
                if (e >= e1) continue;
                while (e >= re && g + 1 < G) {
                    rs = re, re = egoff[++g + 1];
                    fs = fgoff[g], L = fgoff[g + 1] - fs;
                }
                const uint64_t p = e - rs;
                if (p < L) {
                    const uint32_t ch = ascii[fs + p];
                    const uint32_t c = base_code(ch);
                    out[i] = (uint8_t)c;
                    if (c > 3 && ch != 'N' && first == ~0ull) first = fs + p;
                } else if (p > L) {
                    const uint32_t c = base_code(ascii[fs + 2 * L - p]);
                    out[i] = (uint8_t)(c > 3 ? 4u : 3u - c);
                }
            }
        }
        if (e1 - e0 == kExpandRun) {  // (e0 is a multiple of 16: one aligned 16-B store)
            uint4 v;
            v.x = out[0] | out[1] << 8 | out[2] << 16 | (uint32_t)out[3] << 24;
            v.y = out[4] | out[5] << 8 | out[6] << 16 | (uint32_t)out[7] << 24;
            v.z = out[8] | out[9] << 8 | out[10] << 16 | (uint32_t)out[11] << 24;
            v.w = out[12] | out[13] << 8 | out[14] << 16 | (uint32_t)out[15] << 24;
            *(uint4 *)(codes + e0) = v;
        } else {
#pragma unroll
            for (int i = 0; i < kExpandRun; i++)
                if (e0 + i < e1) codes[e0 + i] = out[i];
        }
    }
    if (first != ~0ull) atomicMin(bad, first);
}

__global__ void k_fill_u64(uint64_t *p, uint64_t n, uint64_t v) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}

// Insert (or find) a key; returns its slot.  Slots only go EMPTY -> key, so a
// stale plain load can only show EMPTY, which the CAS then corrects.
template <int NW>
__device__ uint64_t table_insert(Slot<NW> *t, uint64_t cap, const Key<NW> &k, uint64_t home, uint32_t &fresh,
                                 uint32_t *err) {
    uint64_t pos = home;
    if constexpr (NW == 1) {
        for (uint64_t it = 0; it < cap; it++) {
            uint64_t cur = t[pos].key[0];
            if (cur == k.w[0]) return pos;
            if (cur == EMPTY) {
                uint64_t old = atomicCAS((unsigned long long *)&t[pos].key[0], EMPTY, k.w[0]);
                if (old == EMPTY) {
                    fresh++;
                    return pos;
                }
                if (old == k.w[0]) return pos;
            }
            pos = (pos + 1 == cap) ? 0 : pos + 1;
        }
    } else {
        // multi-word keys: the top word doubles as a lock (EMPTY -> BUSY -> key)
        uint32_t spins = 0;
        for (uint64_t it = 0; it < cap;) {
            uint64_t cur = __hip_atomic_load(&t[pos].key[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == BUSY) {
                if (++spins > (1u << 26)) break;
                __builtin_amdgcn_s_sleep(1);
                continue;
            }
            if (cur == EMPTY) {
                uint64_t old = atomicCAS((unsigned long long *)&t[pos].key[0], EMPTY, BUSY);
                if (old == EMPTY) {
#pragma unroll
                    for (int j = 1; j < NW; j++) st_agent(&t[pos].key[j], k.w[j]);
                    __hip_atomic_store(&t[pos].key[0], k.w[0], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    fresh++;
                    return pos;
                }
                continue;  // someone claimed it: look again
            }
            if (cur == k.w[0]) {
                bool eq = true;
#pragma unroll
                for (int j = 1; j < NW; j++) eq &= (ld_agent(&t[pos].key[j]) == k.w[j]);
                if (eq) return pos;
            }
            pos = (pos + 1 == cap) ? 0 : pos + 1;
            it++;
        }
    }
    atomicOr(err, 1u);
    return ~0ull;
}

// Build bookkeeping lives in the slot itself until the slots are final
// (one random line per window instead of four arrays): during pass 1
//   slot.cls  = ~(last genome + 1)   (0xFFFFFFFF: none yet; atomicMin keeps the latest)
//   slot.tpos = ~(genomes so far)    (deg, counted down)
// Genomes are inserted one launch each in FASTA order, so within a launch all
// windows carry the same g and the thread whose atomicMin lowers cls is the
// only one to count g for that slot; a singleton's genome is its last one.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// Pass 1 over one genome: insert windows, count distinct genomes per slot;
// new keys are counted per wave (one atomic per wave, not per key).
template <int NW>
__global__ void k_build_insert(const uint8_t *__restrict__ codes, uint64_t gstart, uint64_t nwin, int k,
                               uint64_t mask0, uint32_t g, Slot<NW> *table, HomeCfg hc, unsigned long long *n_kmers,
                               uint32_t *err, int wpt) {
    const uint64_t cap = hc.cap;
    const uint64_t w0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * wpt;
    uint32_t fresh = 0;
    if (w0 < nwin) {
        const uint64_t w1 = min(w0 + (uint64_t)wpt, nwin);
        const uint8_t *s = codes + gstart + w0;
        Key<NW> key;
#pragma unroll
        for (int j = 0; j < NW; j++) key.w[j] = 0;
        int run = 0;
        for (int i = 0; i < k - 1; i++) {
            uint32_t c = s[i];
            run = c > 3 ? 0 : run + 1;
            key_push(key, c & 3, mask0);
        }
        const uint32_t mark = ~(g + 1);
        for (uint64_t w = w0; w < w1; w++) {
            uint32_t c = s[w - w0 + k - 1];
            run = c > 3 ? 0 : run + 1;
            key_push(key, c & 3, mask0);
            if (run < k) continue;  // window contains a non-ACGT base (src/kmer.py:145)
            const uint64_t slot = table_insert<NW>(table, cap, key, home_of(key, key_hash(key), hc), fresh, err);
            if (slot == ~0ull) break;
            if (atomicMin(&table[slot].cls, mark) > mark) atomicSub(&table[slot].tpos, 1u);
        }
    }
    fresh = wave_sum_u32(fresh);
    if (lane_id() == 0 && fresh) atomicAdd(n_kmers, (unsigned long long)fresh);
}

// Single-word keys (k <= 31), batched: a thread makes the keys of kInsBatch
// windows first and loads their home slots (key + bookkeeping word, 16 B)
// together -- kInsBatch random lines in flight instead of one chain of
// dependent ones (a genome launch fills only ~2 waves per SIMD) -- then
// settles each window: found, claimed (CAS EMPTY -> key) or probed on; and
// counts g for the slot with ONE 64-bit CAS of the bookkeeping word
// {cls = ~(last genome + 1), tpos = ~genomes} (round 5: atomicMin + atomicSub).
// A stale plain load can only show EMPTY or an older (larger) cls: the CASes
// correct both.  Exact for the same reason as k_build_insert: every thread of a
// launch carries the same g.
constexpr int kInsBatch = 8;
__device__ __forceinline__ uint64_t *meta_of(Slot<1> *t, uint64_t pos) { return (uint64_t *)&t[pos].cls; }

// Count genome `mark` for the slot at pos once: (cls, tpos) -> (mark, tpos - 1)
// unless cls is already <= mark.  Returns the genomes listed before g (~old
// tpos), or ~0u when g was counted already.
__device__ __forceinline__ uint32_t count_genome(Slot<1> *t, uint64_t pos, uint64_t m, uint32_t mark) {
    while ((uint32_t)m > mark) {
        const uint64_t nv = ((uint64_t)((uint32_t)(m >> 32) - 1u) << 32) | mark;
        const uint64_t old = atomicCAS((unsigned long long *)meta_of(t, pos), (unsigned long long)m,
                                       (unsigned long long)nv);
        if (old == m) return ~(uint32_t)(m >> 32);
        m = old;
    }
    return ~0u;
}

__global__ __launch_bounds__(256) void k_build_insert1(const uint8_t *__restrict__ codes, uint64_t gstart,
                                                       uint64_t nwin, int k, uint64_t mask0, uint32_t g,
                                                       Slot<1> *table, HomeCfg hc, unsigned long long *n_kmers,
                                                       uint32_t *err, int wpt, uint32_t *__restrict__ lpos) {
    const uint64_t cap = hc.cap;
    const uint64_t w0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * wpt;
    uint32_t fresh = 0;
    if (w0 < nwin) {
        const uint64_t w1 = min(w0 + (uint64_t)wpt, nwin);
        const uint8_t *s = codes + gstart + w0;
        Key<1> key;
        key.w[0] = 0;
        int run = 0;
        for (int i = 0; i < k - 1; i++) {
            const uint32_t c = s[i];
            run = c > 3 ? 0 : run + 1;
            key_push(key, c & 3, mask0);
        }
        const uint32_t mark = ~(g + 1);
        for (uint64_t wb = w0; wb < w1; wb += kInsBatch) {
            uint64_t kk[kInsBatch], hp[kInsBatch];
            uint32_t ok = 0;
#pragma unroll
            for (int i = 0; i < kInsBatch; i++) {
                kk[i] = 0, hp[i] = 0;
                if (wb + i < w1) {
                    const uint32_t c = s[wb + i - w0 + k - 1];
                    run = c > 3 ? 0 : run + 1;
                    key_push(key, c & 3, mask0);
                    if (run >= k) {  // (a window with a non-ACGT base is skipped, src/kmer.py:145)
                        kk[i] = key.w[0];
                        hp[i] = home_of(key, key_hash(key), hc);
                        ok |= 1u << i;
                    }
                }
            }
            ulonglong2 sv[kInsBatch];
#pragma unroll
            for (int i = 0; i < kInsBatch; i++)
                if (ok >> i & 1) sv[i] = *(const ulonglong2 *)&table[hp[i]];
            // the claims of the windows whose home slot is EMPTY, issued together
            uint64_t got[kInsBatch];
#pragma unroll
            for (int i = 0; i < kInsBatch; i++)
                got[i] = (ok >> i & 1) && sv[i].x == EMPTY
                             ? atomicCAS((unsigned long long *)&table[hp[i]].key[0], EMPTY, kk[i])
                             : sv[i].x;
            // settle every window's slot (probing on past other keys: rare at the build's load)
            uint64_t pos[kInsBatch], m[kInsBatch];
            uint32_t claimed = 0;  // fresh keys: their bookkeeping word is stored, not CASed (below)
#pragma unroll
            for (int i = 0; i < kInsBatch; i++) {
                pos[i] = hp[i], m[i] = sv[i].y;
                if (!(ok >> i & 1)) continue;
                if (sv[i].x == EMPTY && got[i] == EMPTY) {  // claimed: a fresh key
                    fresh++;
                    m[i] = ~0ull;
                    claimed |= 1u << i;
                    continue;
                }
                if (got[i] == kk[i]) {
                    if (sv[i].x == EMPTY) m[i] = ld_agent(meta_of(table, pos[i]));  // (claimed by a sibling window)
                    continue;
                }
                bool found = false;
                uint64_t p = pos[i];
                for (uint64_t it = 0; it < cap; it++) {
                    p = (p + 1 == cap) ? 0 : p + 1;
                    const ulonglong2 v = *(const ulonglong2 *)&table[p];
                    uint64_t mm = v.y;
                    if (v.x == EMPTY) {
                        const uint64_t o = atomicCAS((unsigned long long *)&table[p].key[0], EMPTY, kk[i]);
                        if (o == EMPTY) {
                            fresh++;
                            mm = ~0ull;
                            found = true;
                            claimed |= 1u << i;
                        } else if (o == kk[i]) {
                            mm = ld_agent(meta_of(table, p));
                            found = true;
                        }
                    } else if (v.x == kk[i]) {
                        found = true;
                    }
                    if (found) {
                        pos[i] = p, m[i] = mm;
                        break;
                    }
                }
                if (!found) {
                    atomicOr(err, 1u);
                    ok &= ~(1u << i);
                }
            }
            // count g for every slot: a key this thread claimed gets its word
            // {g, one genome} by a plain store -- only windows of the same
            // genome can race for it, and they write or CAS that same value
            // (a third of the pass's atomics: one per distinct k-mer) -- the
            // others' CASes issued together, then the (rare) failed ones again
            // one by one
            uint64_t old[kInsBatch];
            uint32_t want = 0;
#pragma unroll
            for (int i = 0; i < kInsBatch; i++) {
                old[i] = m[i];
                if (claimed >> i & 1) {
                    *meta_of(table, pos[i]) = ((uint64_t)0xFFFFFFFEu << 32) | mark;
                    continue;
                }
                if ((ok >> i & 1) && (uint32_t)m[i] > mark) {
                    want |= 1u << i;
                    const uint64_t nv = ((uint64_t)((uint32_t)(m[i] >> 32) - 1u) << 32) | mark;
                    old[i] = atomicCAS((unsigned long long *)meta_of(table, pos[i]), (unsigned long long)m[i],
                                       (unsigned long long)nv);
                }
            }
            // (lpos: each window's place in its slot's genome list -- the
            // genomes counted before g -- when this window counted g, else
            // ~0u: pass 2 then appends without a CAS, k_build_fill1)
            uint32_t lp[kInsBatch];
#pragma unroll
            for (int i = 0; i < kInsBatch; i++) {
                lp[i] = (claimed >> i & 1) ? 0u : ~0u;
                if (want >> i & 1)
                    lp[i] = old[i] == m[i] ? ~(uint32_t)(m[i] >> 32) : count_genome(table, pos[i], old[i], mark);
            }
            if (lpos) {
#pragma unroll
                for (int i = 0; i < kInsBatch; i++)
                    if (wb + i < w1) lpos[gstart + wb + i] = lp[i];
            }
        }
    }
    fresh = wave_sum_u32(fresh);
    if (lane_id() == 0 && fresh) atomicAdd(n_kmers, (unsigned long long)fresh);
}

// Distinct k-mer estimate (HyperLogLog, 2^16 registers, ~0.4 % error) of one
// genome's windows, to size the table of references whose windows would not
// fit at the default load (e.g. 2000 x 4 Mbp: 8 G windows, ~3.8 G distinct).
constexpr int kHllBits = 16;
template <int NW>
__global__ void k_hll(const uint8_t *__restrict__ codes, uint64_t gstart, uint64_t nwin, int k, uint64_t mask0,
                      uint32_t *reg) {
    uint64_t w0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kRun;
    if (w0 >= nwin) return;
    uint64_t w1 = min(w0 + (uint64_t)kRun, nwin);
    const uint8_t *s = codes + gstart + w0;
    Key<NW> key;
#pragma unroll
    for (int j = 0; j < NW; j++) key.w[j] = 0;
    int run = 0;
    for (int i = 0; i < k - 1; i++) {
        uint32_t c = s[i];
        run = c > 3 ? 0 : run + 1;
        key_push(key, c & 3, mask0);
    }
    for (uint64_t w = w0; w < w1; w++) {
        uint32_t c = s[w - w0 + k - 1];
        run = c > 3 ? 0 : run + 1;
        key_push(key, c & 3, mask0);
        if (run < k) continue;  // (the index skips these windows too)
        const uint64_t h = fmix64(key_hash(key) ^ 0x243F6A8885A308D3ull);
        const uint32_t r = (uint32_t)(h >> (64 - kHllBits));
        const uint32_t rho = (uint32_t)__builtin_clzll((h << kHllBits) | (1ull << (kHllBits - 1))) + 1;
        if (reg[r] < rho) atomicMax(&reg[r], rho);  // (a stale plain load only costs an atomic)
    }
}

// Singletons -> final slot values; multi slots -> list storage.  Each block
// owns one contiguous range of slots: it first sums the list sizes of its
// multi slots and takes its storage with ONE atomic (a bump per wave made
// ~10^7 same-address atomics on C5 and cost 144 ms on C2), then hands out
// offsets inside the range by block-wide scans.
// Singletons -> final slot values (cls = the genome, tpos reset); multi slots
// -> list storage, cls and tpos reset for pass 2 (tpos then counts the list
// down again, so it holds ~deg once the lists are full).
template <int NW>
__global__ __launch_bounds__(256) void k_build_prep(Slot<NW> *table, uint64_t cap, uint64_t *off,
                                                    unsigned long long *bump, unsigned long long *n_multi,
                                                    int keep_deg) {
    __shared__ unsigned long long s_red[2][4];
    __shared__ unsigned long long s_base;
    __shared__ uint32_t s_wave[4];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const uint64_t per = ((cap + gridDim.x - 1) / gridDim.x + 255) & ~255ull;
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = min(cap, lo + per);
    if (lo >= hi) return;
    // phase A: this range's list storage and multi slots (deg is 0 at empty slots: tpos = ~0)
    unsigned long long tot = 0, nm = 0;
    for (uint64_t s = lo + threadIdx.x; s < hi; s += 256) {
        const uint32_t d = ~table[s].tpos;
        if (d >= 2) tot += d, nm++;
    }
    for (int o = 32; o > 0; o >>= 1) {
        tot += __shfl_down(tot, o);
        nm += __shfl_down(nm, o);
    }
    if (lane == 0) s_red[0][wv] = tot, s_red[1][wv] = nm;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long T = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
        const unsigned long long M = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
        s_base = T ? atomicAdd(bump, T) : 0ull;
        if (M) atomicAdd(n_multi, M);
    }
    __syncthreads();
    unsigned long long run = s_base;
    // phase B: singletons get their class, multi slots their list offsets
    for (uint64_t b = lo; b < hi; b += 256) {
        const uint64_t s = b + threadIdx.x;
        uint32_t d = 0;
        if (s < hi && table[s].key[0] != EMPTY) {
            d = ~table[s].tpos;
            if (d == 1) {
                table[s].cls = ~table[s].cls - 1;  // the only genome = the last one
                table[s].tpos = 0xFFFFFFFFu;
                d = 0;
            }
        }
        const uint32_t incl = wave_incl_scan(d);
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            before += i < wv ? s_wave[i] : 0u;
            total += s_wave[i];
        }
        if (d >= 2) {
            off[s] = run + before + incl - d;
            table[s].cls = 0xFFFFFFFFu;
            if (!keep_deg) table[s].tpos = 0xFFFFFFFFu;  // (keep_deg: pass 2 appends by the windows' lpos)
        }
        run += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
}

// Pass 2 over one genome: append g to the genome list of every multi slot
// (singletons already hold their genome, cls < G; multi slots hold ~(last
// genome + 1) >= 2^32 - 2^20 > G while their lists fill).
template <int NW>
__global__ void k_build_fill(const uint8_t *__restrict__ codes, uint64_t gstart, uint64_t nwin, int k,
                             uint64_t mask0, uint32_t g, Slot<NW> *table, HomeCfg hc, uint32_t G,
                             const uint64_t *off, uint32_t *lists, int wpt) {
    const uint64_t cap = hc.cap;
    uint64_t w0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * wpt;
    if (w0 >= nwin) return;
    uint64_t w1 = min(w0 + (uint64_t)wpt, nwin);
    const uint8_t *s = codes + gstart + w0;
    Key<NW> key;
#pragma unroll
    for (int j = 0; j < NW; j++) key.w[j] = 0;
    int run = 0;
    for (int i = 0; i < k - 1; i++) {
        uint32_t c = s[i];
        run = c > 3 ? 0 : run + 1;
        key_push(key, c & 3, mask0);
    }
    const uint32_t mark = ~(g + 1);
    for (uint64_t w = w0; w < w1; w++) {
        uint32_t c = s[w - w0 + k - 1];
        run = c > 3 ? 0 : run + 1;
        key_push(key, c & 3, mask0);
        if (run < k) continue;
        uint64_t slot;
        uint32_t cls, tpos;
        if (!table_find<NW>(table, cap, key, home_of(key, key_hash(key), hc), slot, cls, tpos)) continue;
        if (cls < G) continue;  // a singleton
        if (atomicMin(&table[slot].cls, mark) > mark) {
            const uint32_t p = ~atomicSub(&table[slot].tpos, 1u);  // genomes listed before g
            lists[off[slot] + p] = g;
        }
    }
}

// Pass 2 for single-word keys, batched like k_build_insert1: the windows'
// slots loaded together, then each multi slot's genome list appended with one
// CAS of its bookkeeping word (cls = ~(last genome + 1), tpos = ~listed).
__global__ __launch_bounds__(256) void k_build_fill1(const uint8_t *__restrict__ codes, uint64_t gstart,
                                                     uint64_t nwin, int k, uint64_t mask0, uint32_t g,
                                                     Slot<1> *table, HomeCfg hc, uint32_t G,
                                                     const uint64_t *__restrict__ off, uint32_t *lists, int wpt,
                                                     const uint32_t *__restrict__ lpos) {
    const uint64_t cap = hc.cap;
    const uint64_t w0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * wpt;
    if (w0 >= nwin) return;
    const uint64_t w1 = min(w0 + (uint64_t)wpt, nwin);
    const uint8_t *s = codes + gstart + w0;
    Key<1> key;
    key.w[0] = 0;
    int run = 0;
    for (int i = 0; i < k - 1; i++) {
        const uint32_t c = s[i];
        run = c > 3 ? 0 : run + 1;
        key_push(key, c & 3, mask0);
    }
    const uint32_t mark = ~(g + 1);
    for (uint64_t wb = w0; wb < w1; wb += kInsBatch) {
        uint64_t kk[kInsBatch], hp[kInsBatch];
        uint32_t ok = 0, lp[kInsBatch];
#pragma unroll
        for (int i = 0; i < kInsBatch; i++) {
            kk[i] = 0, hp[i] = 0, lp[i] = ~0u;
            if (wb + i < w1) {
                const uint32_t c = s[wb + i - w0 + k - 1];
                run = c > 3 ? 0 : run + 1;
                key_push(key, c & 3, mask0);
                if (lpos) lp[i] = lpos[gstart + wb + i];
                // (with lpos: only the window that counted g for its slot appends it)
                if (run >= k && (!lpos || lp[i] != ~0u)) {
                    kk[i] = key.w[0];
                    hp[i] = home_of(key, key_hash(key), hc);
                    ok |= 1u << i;
                }
            }
        }
        if (lpos) {  // the list places pass 1 took: no CAS, the slot found and its list written
            if (!ok) continue;
            ulonglong2 sv[kInsBatch];
#pragma unroll
            for (int i = 0; i < kInsBatch; i++)
                if (ok >> i & 1) sv[i] = *(const ulonglong2 *)&table[hp[i]];
#pragma unroll
            for (int i = 0; i < kInsBatch; i++) {
                if (!(ok >> i & 1)) continue;
                uint64_t p = hp[i], cur = sv[i].x;
                uint32_t cls = (uint32_t)sv[i].y;
                while (cur != kk[i] && cur != EMPTY) {
                    p = (p + 1 == cap) ? 0 : p + 1;
                    const ulonglong2 v = *(const ulonglong2 *)&table[p];
                    cur = v.x, cls = (uint32_t)v.y;
                }
                if (cur == kk[i] && cls >= G) lists[off[p] + lp[i]] = g;  // (multi slots only)
            }
            continue;
        }
        ulonglong2 sv[kInsBatch];
#pragma unroll
        for (int i = 0; i < kInsBatch; i++)
            if (ok >> i & 1) sv[i] = *(const ulonglong2 *)&table[hp[i]];
        uint64_t pos[kInsBatch], m[kInsBatch];
        uint32_t want = 0;
#pragma unroll
        for (int i = 0; i < kInsBatch; i++) {
            pos[i] = hp[i], m[i] = sv[i].y;
            if (!(ok >> i & 1)) continue;
            uint64_t cur = sv[i].x;
            while (cur != kk[i] && cur != EMPTY) {  // (every window's key is in the table after pass 1)
                pos[i] = (pos[i] + 1 == cap) ? 0 : pos[i] + 1;
                const ulonglong2 v = *(const ulonglong2 *)&table[pos[i]];
                cur = v.x, m[i] = v.y;
            }
            // multi slots not yet holding g (a singleton's genome is in cls already)
            if (cur == kk[i] && (uint32_t)m[i] >= G && (uint32_t)m[i] > mark) want |= 1u << i;
        }
        // the batch's list appends: their CASes issued together, the (rare)
        // failed ones again one by one
        uint64_t old[kInsBatch];
#pragma unroll
        for (int i = 0; i < kInsBatch; i++) {
            old[i] = m[i];
            if (want >> i & 1) {
                const uint64_t nv = ((uint64_t)((uint32_t)(m[i] >> 32) - 1u) << 32) | mark;
                old[i] = atomicCAS((unsigned long long *)meta_of(table, pos[i]), (unsigned long long)m[i],
                                   (unsigned long long)nv);
            }
        }
#pragma unroll
        for (int i = 0; i < kInsBatch; i++) {
            if (!(want >> i & 1)) continue;
            const uint32_t p = old[i] == m[i] ? ~(uint32_t)(m[i] >> 32) : count_genome(table, pos[i], old[i], mark);
            if (p != ~0u) lists[off[pos[i]] + p] = g;
        }
    }
}

__device__ __forceinline__ uint64_t list_hash(const uint32_t *l, uint32_t n) {
    uint64_t h = fmix64(0x51ED27C3A9F0B1D5ull ^ n);
    for (uint32_t i = 0; i < n; i++) h = fmix64(h ^ ((uint64_t)l[i] * 0x9E3779B97F4A7C15ull + i));
    return h >> 1;  // < 2^63: never EMPTY
}

// (after pass 2: a multi slot has cls >= G and tpos = ~deg)
// A reference has few distinct genome sets and many multi slots (C4: ~10^4 sets,
// ~4 x 10^8 slots), so almost every slot finds its set's entry already there:
// a plain load first, the CAS only on an EMPTY entry (round 5 CASed every
// slot onto a handful of hot words).  cache_pos: the set's entry is left in
// the slot's cls as G + its position (cls is free after pass 2), so that
// k_class_assign needs neither the hash nor the probe again.
template <int NW>
__global__ void k_class_insert(Slot<NW> *table, uint64_t cap, uint32_t G, const uint64_t *off,
                               const uint32_t *lists, uint64_t *cs_key, uint64_t *cs_rep, uint64_t cs_cap,
                               uint32_t *err, int cache_pos) {
    uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; s < cap; s += stride) {
        if (table[s].key[0] == EMPTY || table[s].cls < G) continue;
        uint64_t h = list_hash(lists + off[s], ~table[s].tpos);
        uint64_t pos = home_slot(fmix64(h), cs_cap);
        uint64_t it = 0;
        for (; it < cs_cap; it++) {
            uint64_t cur = ld_agent(&cs_key[pos]);
            if (cur == EMPTY) {
                cur = atomicCAS((unsigned long long *)&cs_key[pos], EMPTY, h);
                if (cur == EMPTY) {
                    cs_rep[pos] = s;
                    break;
                }
            }
            if (cur == h) break;
            pos = (pos + 1 == cs_cap) ? 0 : pos + 1;
        }
        if (it == cs_cap)
            atomicOr(err, 4u);
        else if (cache_pos)
            table[s].cls = G + (uint32_t)pos;
    }
}

template <int NW>
__global__ void k_class_number(const uint64_t *cs_key, const uint64_t *cs_rep, uint32_t *cs_id, uint64_t cs_cap,
                               const Slot<NW> *table, uint32_t *class_size, uint64_t *class_off, uint64_t *rep_of,
                               unsigned long long *n_cls, unsigned long long *bump) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; e < cs_cap; e += stride) {
        if (cs_key[e] == EMPTY) continue;
        uint64_t id = atomicAdd(n_cls, 1ull);
        uint64_t rep = cs_rep[e];
        uint32_t d = ~table[rep].tpos;
        cs_id[e] = (uint32_t)id;
        class_size[id] = d;
        class_off[id] = atomicAdd(bump, (unsigned long long)d + 1);  // record = [size, genomes...]
        rep_of[id] = rep;
    }
}

__global__ void k_class_copy(uint64_t n_cls, const uint64_t *rep_of, const uint32_t *class_size,
                             const uint64_t *class_off, const uint64_t *off, const uint32_t *lists,
                             uint32_t *class_genomes) {
    uint64_t c = blockIdx.x;
    for (; c < n_cls; c += gridDim.x) {
        const uint32_t *src = lists + off[rep_of[c]];
        uint32_t *dst = class_genomes + class_off[c];
        if (threadIdx.x == 0) dst[0] = class_size[c];
        for (uint32_t i = threadIdx.x; i < class_size[c]; i += blockDim.x) dst[1 + i] = src[i];
    }
}

// G <= 64: one 64-bit membership mask per multi-genome set (dense align path).
__global__ void k_class_masks(uint64_t n_cls, const uint64_t *class_off, const uint32_t *class_genomes,
                              uint64_t *class_mask) {
    uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; c < n_cls; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t *rec = class_genomes + class_off[c];
        uint64_t m = 0;
        for (uint32_t i = 0; i < rec[0]; i++) m |= 1ull << rec[1 + i];
        class_mask[class_off[c]] = m;
    }
}

// (every thread reads and writes its own slot only; the representative's
// size comes from class_size, its list from `lists`)
template <int NW>
__global__ void k_class_assign(Slot<NW> *table, uint64_t cap, const uint64_t *off, const uint32_t *lists,
                               const uint64_t *cs_key, const uint64_t *cs_rep, const uint32_t *cs_id, uint64_t cs_cap,
                               const uint32_t *class_size, const uint64_t *class_off, uint32_t n_genomes,
                               uint32_t *err, int cache_pos) {
    uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; s < cap; s += stride) {
        const Slot<NW> me = table[s];
        if (me.key[0] == EMPTY || me.cls < n_genomes) continue;
        const uint32_t d = ~me.tpos;
        const uint32_t *l = lists + off[s];
        uint64_t pos;
        if (cache_pos) {
            pos = me.cls - n_genomes;  // (k_class_insert left the set's entry there)
        } else {
            const uint64_t h = list_hash(l, d);
            pos = home_slot(fmix64(h), cs_cap);
            while (cs_key[pos] != h) pos = (pos + 1 == cs_cap) ? 0 : pos + 1;
        }
        uint64_t rep = cs_rep[pos];
        const uint32_t id = cs_id[pos];
        bool same = class_size[id] == d;
        const uint32_t *rl = lists + off[rep];
        for (uint32_t i = 0; same && i < d; i++) same = (rl[i] == l[i]);
        if (!same) atomicOr(err, 2u);  // 63-bit list-hash collision: refuse, never merge
        // a multi-genome class id is G + the word offset of its [size, genomes...] record
        table[s].cls = n_genomes + (uint32_t)class_off[id];
        table[s].tpos = 0xFFFFFFFFu;  // (the first occurrence, set by the tiles)
    }
}

template <int NW>
__global__ void k_lookup(const Slot<NW> *table, HomeCfg hc, const uint8_t *kmers, uint64_t n, int k, uint64_t mask0,
                         uint32_t G, const uint32_t *class_genomes, int64_t *cls_out, uint32_t *size_out) {
    const uint64_t cap = hc.cap;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = kmers + i * (uint64_t)k;
    Key<NW> key;
#pragma unroll
    for (int j = 0; j < NW; j++) key.w[j] = 0;
    bool ok = true;
    for (int j = 0; j < k; j++) {
        uint32_t c = base_code(s[j]);
        ok &= c < 4;
        key_push(key, c & 3, mask0);
    }
    uint64_t slot;
    uint32_t cls = 0, tpos = 0;
    if (ok && table_find<NW, true>(table, cap, key, home_of(key, key_hash(key), hc), slot, cls, tpos)) {
        cls_out[i] = cls_of(cls);
        size_out[i] = class_size_of(cls, G, class_genomes);
    } else {
        cls_out[i] = -1;
        size_out[i] = 0;
    }
}

// ---- genome tiling ------------------------------------------------------------

// 32 bases per word, first base in the top bits (the read packing of pa_fast.h);
// non-ACGT codes pack as 0 -- tile_cls marks every window that holds one.
__global__ void k_tile_pack(const uint8_t *__restrict__ codes, uint64_t n, uint64_t *__restrict__ pk,
                            uint64_t nwords) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < nwords; i += stride) {
        uint64_t v = 0;
        const uint64_t b = i * 32;
        if (b + 32 <= n) {
            const uint4 *q = (const uint4 *)(codes + b);  // codes are 16-B aligned (hipMalloc), b % 32 == 0
            const uint4 x = q[0], y = q[1];
            const uint32_t wds[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
            for (int d = 0; d < 8; d++)
#pragma unroll
                for (int j = 0; j < 4; j++) v = (v << 2) | ((wds[d] >> (8 * j)) & 3u);
        } else {
            for (int j = 0; j < 32; j++) v = (v << 2) | (b + j < n ? (uint64_t)(codes[b + j] & 3u) : 0ull);
        }
        pk[i] = v;
    }
}

// Class of the k-mer starting at every genome window (tile_cls is
// pre-filled with NONE, which stays at windows with non-ACGT bases), and the
// key's first occurrence: slot.tpos = the smallest position of the key inside
// its first genome (FASTA order: the specific genome, or the first of its set),
// concatenated while the reference is < 2^32 bases, else genome-local so that
// references of any total length tile (the concatenated position is then
// goff[first genome] + tpos; pad::first_pos).
// Tile classes and first occurrences (k_tile_cls_all), every genome in ONE
// launch (they do not depend on the genomes' order): thread T takes chunk T -
// tstart[g] of genome g, the last genome with tstart[g] <= T (tstart: the
// genomes' first chunks, prefix sums of ceil(windows / wpt)); windows never
// cross genomes.  C5's 1200 launches of 0.23 ms became one.
template <int NW>
__global__ void k_tile_cls_all(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ goff,
                               const uint64_t *__restrict__ tstart, uint32_t G, int k, uint64_t mask0,
                               Slot<NW> *table, HomeCfg hc, uint32_t *tile_cls,
                               const uint32_t *__restrict__ class_genomes, int local, int wpt) {
    const uint64_t T = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (T >= tstart[G]) return;
    uint32_t lo = 0, hi = G;  // tstart[lo] <= T < tstart[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tstart[mid] <= T)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t g = lo;
    const uint64_t gstart = goff[g], nwin = goff[g + 1] - gstart - (uint64_t)k + 1;
    const uint64_t w0 = (T - tstart[g]) * (uint64_t)wpt;
    if (w0 >= nwin) return;
    const uint64_t w1 = min(w0 + (uint64_t)wpt, nwin);
    const uint8_t *s = codes + gstart + w0;
    Key<NW> key;
#pragma unroll
    for (int j = 0; j < NW; j++) key.w[j] = 0;
    int run = 0;
    for (int i = 0; i < k - 1; i++) {
        uint32_t c = s[i];
        run = c > 3 ? 0 : run + 1;
        key_push(key, c & 3, mask0);
    }
    for (uint64_t w = w0; w < w1; w++) {
        uint32_t c = s[w - w0 + k - 1];
        run = c > 3 ? 0 : run + 1;
        key_push(key, c & 3, mask0);
        if (run < k) continue;
        uint64_t slot;
        uint32_t cls, tpos;
        if (table_find<NW, true>(table, hc.cap, key, home_of(key, key_hash(key), hc), slot, cls, tpos)) {
            tile_cls[gstart + w] = cls;
            if (local) {
                const uint32_t fg = cls < G ? cls : class_genomes[cls - G + 1];
                if (fg == g && tpos > (uint32_t)w) atomicMin(&table[slot].tpos, (uint32_t)w);
            } else if (tpos > (uint32_t)(gstart + w)) {
                atomicMin(&table[slot].tpos, (uint32_t)(gstart + w));
            }
        }
    }
}

// First occurrences as concatenated positions for references of 2^32 .. 2^33
// bases (tiled with genome-local tpos, k_tile_cls_all): tpos = the low 32
// bits, bit 31 of cls = bit 32 (pad::first_pos).  The lane kernels' anchors
// then need no class-record and goff loads (C4 laid out genome-locally ran
// 5 % slower: profiles/r05/ab_tpos_local.txt).  One pass over the slots.
// The one first occurrence whose low 32 bits are all ones (position 2^32 - 1
// or 2^33 - 1) reads as NONE afterwards: that k-mer then gives no anchor, so a
// read seeded only by it takes the seedless path (k_align_lane_na tests every
// window, a specific k-mer sends the read to the wave kernel) -- slower for
// that read, never a different result.
template <int NW>
__global__ void k_tpos_concat(Slot<NW> *table, uint64_t cap, uint32_t G, const uint32_t *__restrict__ class_genomes,
                              const uint64_t *__restrict__ goff) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        Slot<NW> &s = table[i];
        if (s.key[0] == EMPTY || s.tpos == NONE) continue;
        const uint64_t fo = first_pos(s.cls, s.tpos, G, class_genomes, goff, true);
        s.tpos = (uint32_t)fo;
        s.cls |= (uint32_t)(fo >> 32) << 31;
    }
}

// Local-repeat flags: bit 31 (PA_TILE_REP) of tile_cls[t] marks an indexed
// window whose k-mer starts again at an indexed window within the next
// kTileRepDist positions.  A read walked along the genomes then holds a k-mer
// twice only if one of its walked windows carries the flag (its windows are
// < kTileRepDist apart), which the lane kernel (pa_lane.h) tests instead of
// deduplicating.  One block per 256 positions, keys staged in LDS.
constexpr int kTileRepDist = 255;  // (>= the lane kernels' longest span of windows: 256 windows, pa_lane.h)
// One block per 256 windows and the 255 after them, staged in LDS; round 6:
// instead of comparing every window with each of the next 255 (~500 LDS reads
// per window, VALU-bound: 47 ms for C4's 1 Gbp), the span's keys go into an
// LDS hash of their distinct values, each holding the chain of the positions
// where it occurs; a window then walks only its own key's chain -- one entry
// unless the k-mer repeats.
template <int NW>  // (1: k <= 31, 2: k <= 63, 3: k <= 95 -- the key words compared)
__global__ __launch_bounds__(256) void k_tile_rep(const uint64_t *__restrict__ pk, uint32_t *tile_cls, uint64_t n,
                                                  int k) {
    constexpr int SPAN = 256 + kTileRepDist, HS = 1024;  // (the hash at most half full)
    constexpr uint32_t NIL = 0xFFFFFFFFu;
    __shared__ uint64_t keys[NW][SPAN];
    __shared__ uint32_t valid[SPAN], nxt[SPAN];
    __shared__ uint32_t rep_of[HS], chain[HS];  // a slot's representative position / its latest position
    const int sh = 64 - 2 * k;
    auto same = [&](int a, int b) {
        bool eq = true;
#pragma unroll
        for (int j = 0; j < NW; j++) eq = eq && keys[j][a] == keys[j][b];
        return eq;
    };
    auto slot_of = [&](int i) {
        uint64_t h = keys[0][i];
#pragma unroll
        for (int j = 1; j < NW; j++) h = h * 0x9E3779B97F4A7C15ull ^ keys[j][i];
        return (uint32_t)(fmix64(h) >> 54);  // HS = 2^10
    };
    for (uint64_t b = (uint64_t)blockIdx.x * 256; b < n; b += (uint64_t)gridDim.x * 256) {
        __syncthreads();
        for (int i = threadIdx.x; i < HS; i += 256) rep_of[i] = NIL, chain[i] = NIL;
        for (int i = threadIdx.x; i < SPAN; i += 256) {
            const uint64_t t = b + i;
            const bool ok = t < n && tile_cls[t] != NONE;
            valid[i] = ok;
            if (NW == 1) {
                keys[0][i] = ok ? (get64_at(pk, 2 * t) >> sh) : 0;
            } else {  // the key's words (pa_lane.h row_key)
                const Key<NW> K = ok ? genome_key<NW>(pk, t, k) : Key<NW>{};
#pragma unroll
                for (int j = 0; j < NW; j++) keys[j][i] = K.w[j];
            }
        }
        __syncthreads();
        // every indexed window of the span into the hash: its key's slot (a
        // slot's representative is the first position to claim it), then
        // pushed on the slot's chain
        for (int i = threadIdx.x; i < SPAN; i += 256) {
            if (!valid[i]) continue;
            uint32_t s = slot_of(i);
            for (;;) {
                uint32_t r = rep_of[s];
                if (r == NIL) {
                    r = atomicCAS(&rep_of[s], NIL, (uint32_t)i);
                    if (r == NIL) break;
                }
                if (same((int)r, i)) break;
                s = (s + 1) & (HS - 1);
            }
            nxt[i] = atomicExch(&chain[s], (uint32_t)i);
        }
        __syncthreads();
        const uint64_t t = b + threadIdx.x;
        if (t < n && valid[threadIdx.x]) {
            const int me = threadIdx.x;
            uint32_t s = slot_of(me);
            while (!same((int)rep_of[s], me)) s = (s + 1) & (HS - 1);
            bool rep = false;
            for (uint32_t q = chain[s]; q != NIL && !rep; q = nxt[q]) rep = (int)q > me && (int)q <= me + kTileRepDist;
            if (rep) tile_cls[t] |= PA_TILE_REP;
        }
    }
}

// One-substitution neighbours of every indexed genome window, for the lane
// kernel: bit i of the low half of nb[3 p + b] says whether the k-mer starting
// at p - k + 1 + i with its base at p replaced by the b-th other base
// ((genome base + 1 + b) & 3) is in the index, bit i of the high half whether
// it is there as a specific k-mer.  A read window that matches the genome
// except at one base p is then resolved by one bit -- all k windows around a
// sequencing error by one word -- instead of k table probes; and a read walked
// on a sibling of its genome (a family variant, not an error, at p) learns
// that the variant k-mer is shared, which is all an ambiguous read needs.
// Defined on the 2-bit genome string (N packed as A), for windows that are
// indexed themselves (tile_cls != NONE).
// Two passes: pass 0 probes the 3k neighbours of every window that is its
// k-mer's first occurrence (slot.tpos); pass 1 copies them to every other
// occurrence t of the k-mer, which has the same neighbours: the bits of window
// t sit at the same bit (k - 1 - j) of words 3 (t + j) + b as the first
// occurrence's in words 3 (fo + j) + b, so the copy reads 3k consecutive words
// (~6 128-B lines) instead of probing 3k keys (C5's families repeat about half
// of their windows).
// rc = 1 (tile_rcnb, 32-bit present words): the same for the neighbours'
// REVERSE COMPLEMENTS, for k_align_lane_rc's reverse-strand walk -- a read
// window that is the reverse complement of the genome's k-mer but for one base
// is then resolved by one bit, as a forward one by tile_nb.
// full: 64-bit words, present | specific << 32; else 32-bit words, present
// (nbw: the words in one or two pieces).
//
// k_nb_first is pass 0, in POSITION order: a wave takes 64 consecutive windows
// and walks their 64 k (window, substituted position) pairs ordered by the
// substituted position p, 64 pairs per step, instead of one window per lane
// and one offset j per step.  The neighbours of the windows around one p
// mostly share their minimizer -- the Bloom blocks are chosen by it -- so one
// memory instruction of the wave touches ~7 distinct Bloom blocks instead of
// ~40 (scripts/nb_model.py).  The pair of lane l at step s is the entry
// s 64 + l of the block's decode table (LDS, by p then window); the window's
// key comes from the lane that owns it (a cross-lane read).  Against one
// window per lane, the same bits set by the same atomics, C5: 4.21 -> 3.55 s
// -- the pass is bound by the minimizers' VALU (93 per window) as much as by
// its Bloom lines; listing the filter's positives in LDS and probing them in
// one batch per tile (occupancy 3 instead of 4) measured 4.56 s.
constexpr int kNbFirstChunk = 2;  // steps whose Bloom words are in flight together
__global__ __launch_bounds__(256) void k_nb_first(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ tile_cls,
                                                  uint64_t n, int k, const Slot<1> *__restrict__ table, HomeCfg hc,
                                                  uint32_t G, NbW nbw, int full,
                                                  const uint32_t *__restrict__ class_genomes,
                                                  const uint64_t *__restrict__ goff, int local,
                                                  const uint64_t *__restrict__ bloom, uint32_t bloom_lg, int rc) {
    __shared__ uint16_t pair_of[64 * 31];  // (p - t0) << 6 | window lane, p-major
    for (int q = threadIdx.x; q < 64 + k - 1; q += blockDim.x) {  // one thread per p: its windows
        const int lo = q - k + 1 > 0 ? q - k + 1 : 0, hi = q < 63 ? q : 63;
        int base = 0;  // pairs of the positions before q
        for (int d = 0; d < q; d++) base += (d < 63 ? d : 63) - (d - k + 1 > 0 ? d - k + 1 : 0) + 1;
        for (int l = lo; l <= hi; l++) pair_of[base + (l - lo)] = (uint16_t)((q << 6) | l);
    }
    __syncthreads();
    const int sh = 64 - 2 * k;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t t0 = wave * 64; t0 < n; t0 += n_waves * 64) {
        const uint64_t t = t0 + lane;
        uint64_t K = 0;
        bool first = false;
        if (t < n && tile_cls[t] != NONE) {
            K = get64_at(pk, 2 * t) >> sh;
            Key<1> kk;
            kk.w[0] = K;
            uint64_t slot;
            uint32_t cls, tpos;
            if (table_find<1, true>(table, hc.cap, kk, home_of<1>(kk, key_hash(kk), hc), slot, cls, tpos))
                first = first_pos(cls, tpos, G, class_genomes, goff, local != 0) == t;
        }
        const uint64_t fm = __ballot(first);
        if (!fm) continue;
        for (int s0 = 0; s0 < k; s0 += kNbFirstChunk) {
            uint64_t key[kNbFirstChunk][3], wv[kNbFirstChunk][3], bm[kNbFirstChunk][3];
            uint32_t j_of[kNbFirstChunk], p_of[kNbFirstChunk], pass_bits = 0;
#pragma unroll
            for (int c = 0; c < kNbFirstChunk; c++) {
                const int s = s0 + c;
                const uint32_t e = s < k ? pair_of[s * 64 + lane] : 0u;
                const uint32_t l = e & 63, dp = e >> 6;
                const uint64_t Kw = (uint64_t)__shfl((unsigned long long)K, (int)l);  // (all lanes take part)
                const bool a = s < k && ((fm >> l) & 1ull);
                const int j = (int)dp - (int)l;
                j_of[c] = (uint32_t)j, p_of[c] = a ? dp : ~0u;
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    wv[c][b] = 0, bm[c][b] = 0, key[c][b] = 0;
                    if (a) {
                        const int bs = 2 * (k - 1 - j);
                        const uint64_t cj = (Kw >> bs) & 3;
                        const uint64_t v = Kw ^ ((cj ^ ((cj + 1 + b) & 3)) << bs);
                        key[c][b] = rc ? rc_key(v, k) : v;
                        if (bloom) {
                            uint64_t wi;
                            bloom_word_nb(key[c][b], k, bloom_lg, wi, bm[c][b]);
                            wv[c][b] = bloom[wi];
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < kNbFirstChunk; c++)
#pragma unroll
                for (int b = 0; b < 3; b++)
                    if (p_of[c] != ~0u && (!bloom || (wv[c][b] & bm[c][b]) == bm[c][b])) pass_bits |= 1u << (3 * c + b);
#pragma unroll
            for (int c = 0; c < kNbFirstChunk; c++) {
                const uint32_t act = (pass_bits >> (3 * c)) & 7u;
                if (!act) continue;
                uint32_t cls3[3];
                const uint32_t f = probe_lines<3>(table, hc, key[c], cls3, act);
                const uint64_t p = t0 + p_of[c];
                const int j = (int)j_of[c];
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    if (!((f >> b) & 1u)) continue;
                    if (full)
                        atomicOr(nbw.word<unsigned long long>(3 * p + b), (cls3[b] < G ? 0x100000001ull : 1ull) << (k - 1 - j));
                    else
                        atomicOr(nbw.word<uint32_t>(3 * p + b), 1u << (k - 1 - j));
                }
            }
        }
    }
}

// Pass 1 of the neighbour bits (k_nb_first states the scheme) on its own (the probe loop of pass 0 holds 108 VGPRs;
// this copy needs a third of them, so twice the waves hide its latency):
// every occurrence t of a k-mer other than its first copies the first
// occurrence's bits, k consecutive words per substitution (bit k - 1 - j of
// word 3 (fo + j) + b to the same bit of word 3 (t + j) + b).
__global__ void k_nb_copy(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ tile_cls, uint64_t n, int k,
                          const Slot<1> *__restrict__ table, HomeCfg hc, uint32_t G, NbW nbw, int full,
                          const uint32_t *__restrict__ class_genomes, const uint64_t *__restrict__ goff, int local) {
    const int sh = 64 - 2 * k;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        if (tile_cls[t] == NONE) continue;
        Key<1> kk;
        kk.w[0] = get64_at(pk, 2 * t) >> sh;
        uint64_t slot;
        uint32_t cls, tpos;
        if (!table_find<1, true>(table, hc.cap, kk, home_of<1>(kk, key_hash(kk), hc), slot, cls, tpos)) continue;
        const uint64_t fo = first_pos(cls, tpos, G, class_genomes, goff, local != 0);
        if (fo == t) continue;
        for (int j = 0; j < k; j++) {
#pragma unroll
            for (int b = 0; b < 3; b++) {
                if (full) {
                    const unsigned long long m = *nbw.word<unsigned long long>(3 * (fo + j) + b) & (0x100000001ull << (k - 1 - j));
                    if (m) atomicOr(nbw.word<unsigned long long>(3 * (t + j) + b), m);
                } else {
                    const uint32_t m = *nbw.word<uint32_t>(3 * (fo + j) + b) & (1u << (k - 1 - j));
                    if (m) atomicOr(nbw.word<uint32_t>(3 * (t + j) + b), m);
                }
            }
        }
    }
}

// The same for two- and three-word keys (31 < k <= 95: pa_device.h
// bloom_word2 / bloom_word3).
template <int NW = 2>
__global__ void k_bloom_build2(const Slot<NW> *__restrict__ table, uint64_t cap, uint64_t *bloom, uint32_t lg) {
    static_assert(NW == 2 || NW == 3, "two- or three-word keys");
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        const Slot<NW> s = table[i];
        if (s.key[0] == EMPTY) continue;
        Key<NW> kk;
#pragma unroll
        for (int j = 0; j < NW; j++) kk.w[j] = s.key[j];
        uint64_t w, m;
        if constexpr (NW == 2)
            bloom_word2(kk, lg, w, m);
        else
            bloom_word3(kk, lg, w, m);
        atomicOr((unsigned long long *)&bloom[w], (unsigned long long)m);
    }
}

// Neighbour summaries of three-word keys (63 < k <= 95): nbs holds 4 bits per
// genome position p (8 positions per 32-bit word), bit b set when SOME indexed
// window holding p is, with its base at p replaced by the b-th other base,
// a key of the index.  A k-window word of bits as for k <= 63 would take 48 B
// per base; the summary takes 0.5, and a read window with one mismatch at p
// whose summary bit is clear is absent (the lane walk, pa_lane.h) -- on a
// random or family reference almost every such bit is clear, a set one only
// makes the walk probe that mismatch's windows.  Every indexed window probes
// its 3k neighbours, the build-time Bloom filter (bloom_word3) first.
__global__ void k_nb_sum3(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ tile_cls, uint64_t n, int k,
                          const Slot<3> *__restrict__ table, HomeCfg hc, uint32_t *nbs,
                          const uint64_t *__restrict__ bloom, uint32_t bloom_lg) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        if (tile_cls[t] == NONE) continue;
        const Key<3> K = genome_key<3>(pk, t, k);
        for (int j = 0; j < k; j++) {
            const uint64_t p = t + j;
            uint32_t have = 0;
            for (int b = 0; b < 3; b++) {
                const Key<3> N = key_sub<3>(K, j, k, b);
                if (bloom) {
                    uint64_t w, m;
                    bloom_word3(N, bloom_lg, w, m);
                    if ((bloom[w] & m) != m) continue;
                }
                uint64_t s2;
                uint32_t c2, p2;
                if (table_find<3, true>(table, hc.cap, N, home_of<3>(N, key_hash(N), hc), s2, c2, p2)) have |= 1u << b;
            }
            if (have) atomicOr(&nbs[p >> 3], have << (4 * (p & 7)));
        }
    }
}

// The neighbour bits of two-word keys (31 < k <= 63; k_nb_first states the
// scheme): bit i of nb[3 p + b] says whether the k-mer starting at p - k + 1 +
// i with its base at p replaced by the b-th other base is in the index --
// 64-bit words of present neighbours only (a present one is then probed by the
// lane kernel).  The build-time Bloom filter (bloom_word2) in front of the probes.
__global__ void k_nb_build2(const uint64_t *__restrict__ pk, const uint32_t *__restrict__ tile_cls, uint64_t n, int k,
                            const Slot<2> *__restrict__ table, HomeCfg hc, uint32_t G, unsigned long long *nb,
                            const uint32_t *__restrict__ class_genomes, const uint64_t *__restrict__ goff, int local,
                            int pass, const uint64_t *__restrict__ bloom, uint32_t bloom_lg) {
    const int hb = 2 * k - 64;  // bits of the key's top word
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; t < n; t += stride) {
        if (tile_cls[t] == NONE) continue;
        Key<2> K;
        K.w[1] = get64_at(pk, 2 * t + 2 * k - 64);
        K.w[0] = hb ? get64_at(pk, 2 * t) >> (64 - hb) : 0ull;
        uint64_t slot;
        uint32_t cls, tpos;
        if (!table_find<2, true>(table, hc.cap, K, home_of<2>(K, key_hash(K), hc), slot, cls, tpos)) continue;
        const uint64_t fo = first_pos(cls, tpos, G, class_genomes, goff, local != 0);
        if ((fo == t) != (pass == 0)) continue;
        if (pass == 1) {  // copy the first occurrence's bits of this window
            for (int j = 0; j < k; j++)
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    const unsigned long long m = nb[3 * (fo + j) + b] & (1ull << (k - 1 - j));
                    if (m) atomicOr(&nb[3 * (t + j) + b], m);
                }
            continue;
        }
        for (int j = 0; j < k; j++) {
            const int bs = 2 * (k - 1 - j);  // the base's bit offset in the 2k-bit key
            const int wi = bs >= 64 ? 0 : 1, bo = bs >= 64 ? bs - 64 : bs;
            const uint64_t cj = (K.w[wi] >> bo) & 3;
            for (int b = 0; b < 3; b++) {
                Key<2> N = K;
                N.w[wi] ^= (cj ^ ((cj + 1 + b) & 3)) << bo;
                if (bloom) {
                    uint64_t w, m;
                    bloom_word2(N, bloom_lg, w, m);
                    if ((bloom[w] & m) != m) continue;
                }
                uint64_t s2;
                uint32_t c2, p2;
                if (table_find<2, true>(table, hc.cap, N, home_of<2>(N, key_hash(N), hc), s2, c2, p2))
                    atomicOr(&nb[3 * (t + j) + b], 1ull << (k - 1 - j));
            }
        }
    }
}

// The Bloom filter of the table's keys (pa_device.h bloom_word): one pass over
// the slots, an atomic OR per key.
template <bool NB = false>  // NB: the neighbour-bit build's own filter (bloom_word_nb)
__global__ void k_bloom_build(const Slot<1> *__restrict__ table, uint64_t cap, uint64_t *bloom, uint32_t lg, int k) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        const uint64_t key = table[i].key[0];
        if (key == EMPTY) continue;
        uint64_t w, m;
        if (NB)
            bloom_word_nb(key, k, lg, w, m);
        else
            bloom_word(key, k, lg, w, m);
        atomicOr((unsigned long long *)&bloom[w], (unsigned long long)m);
    }
}

// The reverse-complement plane of the genome tiling, for k_align_lane_na's
// reverse-strand walk (pa_lane.h): bit i of rcp[j] is 0 iff position t = 64 j +
// i starts an indexed window whose reverse complement is NOT a key -- then a
// read window that is the reverse complement of the genome's k-mer at t is
// shown absent without a lookup.  1 where no indexed window starts (N, genome
// end, padding): such a read window is looked up.  One wave per 64 positions,
// the Bloom filter first (most reverse complements are absent), then the table.
__global__ __launch_bounds__(256) void k_tile_rcp(const uint32_t *__restrict__ tile_cls, const uint64_t *__restrict__ pk,
                                                  uint64_t n, int k, const Slot<1> *__restrict__ table, HomeCfg hc,
                                                  const uint64_t *__restrict__ bloom, uint32_t bloom_lg,
                                                  uint64_t *__restrict__ rcp, uint64_t n_blocks) {
    const uint32_t lane = threadIdx.x & 63;
    const int sh = 64 - 2 * k;
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t j = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n_blocks; j += nw) {
        const uint64_t t = 64 * j + lane;
        bool maybe = true;
        if (t < n && tile_cls[t] != NONE) {
            Key<1> kk;
            kk.w[0] = rc_key(get64_at(pk, 2 * t) >> sh, k);
            if (bloom) {
                uint64_t wi, bm;
                bloom_word(kk.w[0], k, bloom_lg, wi, bm);
                maybe = (bloom[wi] & bm) == bm;
            }
            uint64_t slot;
            uint32_t cls, tpos;
            if (maybe) maybe = table_find<1, true>(table, hc.cap, kk, home_of<1>(kk, key_hash(kk), hc), slot, cls, tpos);
        }
        const uint64_t b = __ballot(maybe);
        if (lane == 0) rcp[j] = b;
    }
}

// The minimizer presence bitmap: bit mm_bit(minimizer) of every key (the
// minimizer of bloom_word's block), one pass over the slots.
__global__ void k_mm_build(const Slot<1> *__restrict__ table, uint64_t cap, uint32_t *bits, uint32_t lg, int k) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
        const uint64_t key = table[i].key[0];
        if (key == EMPTY) continue;
        const uint32_t h = mm_bit(k == 31 ? key_minimizer_c<31>(key) : key_minimizer(key, k), lg);
        atomicOr(&bits[h >> 5], 1u << (h & 31));
    }
}

// The lane walk's view of the genomes (pa_lane.h), one 32-B block per 64
// positions j: {2-bit words 2j and 2j+1 of tile_pk (positions 64 j .. 64 j +
// 63), flag plane A, flag plane B}, bit i of a plane <-> position 64 j + i:
// (A,B) = (0,0) no indexed window, (1,0) a multi-genome k-mer, (1,1) a
// specific one, (0,1) a k-mer that repeats within 255 positions (PA_TILE_REP).
// A read's walk needs the bases of [A, A + 150) and the flags of its 120
// windows: 3 or 4 consecutive blocks, 96-128 B -- on gfx950, where every miss
// is a 128-B request, 1.6 lines on average, against 2.6 for the separate
// 2-bit string and plane arrays.  One wave per block, the planes by ballot.
__global__ __launch_bounds__(256) void k_tile_walk(const uint32_t *__restrict__ tile_cls, const uint64_t *__restrict__ pk,
                                                   uint64_t n, uint32_t G, uint64_t *__restrict__ lw, uint64_t n_blocks) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t j = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n_blocks; j += nw) {
        const uint64_t t = 64 * j + lane;
        const uint32_t v = t < n ? tile_cls[t] : NONE;
        const bool ok = v != NONE, rep = ok && (v & PA_TILE_REP);
        const bool spec = ok && !rep && (v & ~PA_TILE_REP) < G;
        const uint64_t a = __ballot(ok && !rep), b = __ballot(rep || spec);
        if (lane < 4) {
            const uint64_t w = lane == 0 ? (64 * j < n ? pk[2 * j] : 0ull)
                             : lane == 1 ? (64 * j + 32 < n ? pk[2 * j + 1] : 0ull)
                             : lane == 2 ? a : b;
            lw[4 * j + lane] = w;
        }
    }
}

// ---- ordered clusters (see probe_past, pa_device.h) --------------------------
// The last pass of a build: every cluster (maximal run of occupied slots,
// cyclic) put in the order of its keys' homes counted from its first slot, by
// one thread per cluster (the slot after an EMPTY one), an insertion sort in
// place.  Only slots move (key, class and first position together); the
// occupied slots stay the same, every key stays at or after its home with no
// EMPTY slot between, so every search finds what it found before.  A key only
// moves back past keys homed after it, which lie inside its own probe span, so
// the work is the sum of the displacements, not the square of a cluster's
// length.  C5's 87 GB table: one read of its slots.
template <int NW>
__global__ void k_table_order(Slot<NW> *table, HomeCfg hc) {
    const uint64_t cap = hc.cap;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < cap; i += stride) {
        if (table[i].key[0] == EMPTY || table[i == 0 ? cap - 1 : i - 1].key[0] != EMPTY) continue;
        auto at = [&](uint64_t t) { return i + t >= cap ? i + t - cap : i + t; };
        auto rel = [&](const Slot<NW> &s) {  // home, counted from the cluster's first slot
            Key<NW> kk;
#pragma unroll
            for (int j = 0; j < NW; j++) kk.w[j] = s.key[j];
            const uint64_t h = home_of<NW>(kk, key_hash(kk), hc);
            return h >= i ? h - i : h + cap - i;
        };
        for (uint64_t t = 1;; t++) {
            const Slot<NW> x = table[at(t)];
            if (x.key[0] == EMPTY) break;
            const uint64_t hx = rel(x);
            uint64_t q = t;
            for (; q > 0; q--) {
                const Slot<NW> y = table[at(q - 1)];
                if (rel(y) <= hx) break;
                table[at(q)] = y;
            }
            if (q != t) table[at(q)] = x;
        }
    }
}

// ---- EXTSIM statistics ------------------------------------------------------

template <int NW>
__global__ void k_extsim_slots(const Slot<NW> *table, uint64_t cap, uint32_t n_genomes, const uint32_t *group_of,
                               uint32_t n_groups, unsigned long long *total, unsigned long long *uniq,
                               unsigned long long *class_count, int use_lds) {
    extern __shared__ unsigned long long sh[];  // [n_groups] totals (singletons: total == uniq increments)
    if (use_lds) {
        for (uint32_t i = threadIdx.x; i < n_groups; i += blockDim.x) sh[i] = 0;
        __syncthreads();
    }
    uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; s < cap; s += stride) {
        if (table[s].key[0] == EMPTY) continue;
        uint32_t c = cls_of(table[s].cls);
        if (c < n_genomes) {
            uint32_t a = group_of[c];
            if (use_lds)
                atomicAdd(&sh[a], 1ull);
            else {
                atomicAdd(&total[a], 1ull);
                atomicAdd(&uniq[a], 1ull);
            }
        } else {
            atomicAdd(&class_count[c - n_genomes], 1ull);  // indexed by record offset
        }
    }
    if (use_lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_groups; i += blockDim.x)
            if (sh[i]) {
                atomicAdd(&total[i], sh[i]);
                atomicAdd(&uniq[i], sh[i]);
            }
    }
}

// One block per multi class: distinct groups of the class, then all ordered pairs.
__global__ void k_extsim_classes(uint64_t n_cls, const uint64_t *class_off, const uint32_t *class_size,
                                 const uint32_t *class_genomes, const uint32_t *group_of, uint32_t n_groups,
                                 const unsigned long long *class_count, unsigned long long *total,
                                 unsigned long long *inter, uint32_t *scratch, uint64_t scratch_stride) {
    __shared__ uint32_t n_distinct;
    for (uint64_t c = blockIdx.x; c < n_cls; c += gridDim.x) {
        unsigned long long nc = class_count[class_off[c]];
        if (nc == 0) continue;
        uint32_t sz = class_size[c];
        const uint32_t *gl = class_genomes + class_off[c] + 1;
        uint32_t *grp = scratch + blockIdx.x * scratch_stride;
        if (threadIdx.x == 0) n_distinct = 0;
        __syncthreads();
        // keep the first occurrence of every group (lists are short; O(sz^2) is fine)
        for (uint32_t i = threadIdx.x; i < sz; i += blockDim.x) {
            uint32_t a = group_of[gl[i]];
            bool first = true;
            for (uint32_t j = 0; j < i && first; j++) first = group_of[gl[j]] != a;
            if (first) grp[atomicAdd(&n_distinct, 1u)] = a;
        }
        __syncthreads();
        uint32_t nd = n_distinct;
        for (uint64_t t = threadIdx.x; t < (uint64_t)nd * nd; t += blockDim.x) {
            uint32_t x = (uint32_t)(t / nd), y = (uint32_t)(t % nd);
            if (x == y)
                atomicAdd(&total[grp[x]], nc);
            else
                atomicAdd(&inter[(uint64_t)grp[x] * n_groups + grp[y]], nc);
        }
        __syncthreads();
    }
}

// ---- synthetic reads --------------------------------------------------------

__device__ __forceinline__ uint64_t rng(uint64_t seed, uint64_t a, uint64_t b) {
    return fmix64(seed * 0xD1B54A32D192ED03ull ^ fmix64(a * 0x9E3779B97F4A7C15ull + b));
}

// Read r = global read first + r: a genome (uniform over those >= len), a start
// (uniform), forward strand -- or, with rc_thresh / foreign_thresh > 0 (the
// robustness workload), the reverse complement of that stretch (the reference
// looks up forward k-mers only, src/kmer.py:423: such reads mostly go
// unmapped) or uniform random bases (an organism absent from the index);
// substitutions at sub_thresh / 2^24 per base; raw-ASCII qualities.
__global__ void k_synth_reads(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ goff,
                              const uint32_t *__restrict__ eligible, uint32_t n_eligible, uint64_t n_reads,
                              uint32_t len, uint64_t first, uint64_t seed, uint32_t sub_thresh, uint32_t rc_thresh,
                              uint32_t foreign_thresh, uint8_t *seq, uint8_t *qual, uint64_t *off,
                              const uint64_t *__restrict__ fwd_len) {  // both-strand index: the forward halves' lengths
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t total = n_reads * len;
    const char acgt[4] = {'A', 'C', 'G', 'T'};
    for (; i < total; i += stride) {
        uint64_t r = i / len;
        uint32_t j = (uint32_t)(i - r * len);
        uint64_t gr = first + r;
        uint64_t h0 = rng(seed, gr, 0xFFFFFFFFull);
        uint32_t g = eligible[(uint32_t)((h0 >> 32) * n_eligible >> 32)];
        uint64_t glen = fwd_len ? fwd_len[g] : goff[g + 1] - goff[g];
        uint64_t start = __umul64hi(rng(seed, gr, 0xFFFFFFFEull), glen - len + 1);
        uint32_t kind = 0;  // 0 forward, 1 reverse complement, 2 foreign
        if (rc_thresh | foreign_thresh) {
            const uint32_t u = (uint32_t)(rng(seed, gr, 0xFFFFFFFDull) >> 40);
            kind = u < foreign_thresh ? 2u : (u < foreign_thresh + rc_thresh ? 1u : 0u);
        }
        uint64_t h = rng(seed, gr, j);
        uint32_t c = kind == 0 ? codes[goff[g] + start + j] : kind == 1 ? codes[goff[g] + start + (len - 1 - j)] : 0u;
        if (c > 3) c = (uint32_t)(h & 3);                       // N in the genome -> random base
        if (kind == 1) c = 3u - c;                              // complement (A-T, C-G)
        if (kind == 2) c = (uint32_t)(rng(seed, gr, j + 0x200000000ull) & 3);
        if ((uint32_t)(h >> 40) < sub_thresh) c = (c + 1 + (uint32_t)((h >> 8) % 3)) & 3;  // substitution
        // raw-ASCII quality: clipped normal(60, 8) via an Irwin-Hall sum of four uniforms
        float u = (float)((h >> 2) & 0xFFF) + (float)((h >> 14) & 0xFFF) + (float)((h >> 26) & 0xFFF) +
                  (float)(rng(seed, gr, j + 0x100000000ull) & 0xFFF);
        float z = (u / 4096.0f - 2.0f) * 1.7320508f;
        int q = (int)rintf(60.0f + 8.0f * z);
        q = q < 35 ? 35 : (q > 74 ? 74 : q);
        seq[i] = (uint8_t)acgt[c];
        qual[i] = (uint8_t)q;
        if (j == 0) off[r] = r * len;
        if (i == total - 1) off[n_reads] = total;
    }
}

// The windows of every genome that has one, in FASTA order (the insert, fill
// and HyperLogLog scans; the tile chunks): f(genome, its first base, windows).
template <class F>
void for_each_genome_windows(const pa_index *idx, int k, F &&f) {
    for (uint32_t g = 0; g < idx->n_genomes; g++) {
        const uint64_t len = idx->h_goff[g + 1] - idx->h_goff[g];
        if (k <= 0 || (uint64_t)k > len) continue;
        f(g, idx->h_goff[g], len - k + 1);
    }
}

// Steps 3 to 6: the table's keys, classes and first occurrences.
template <int NW>
pa_status build_nw(pa_index *idx, hipStream_t st) {
    const uint32_t G = idx->n_genomes;
    const int k = (int)idx->k;
    const int wpt = build_run();
    const uint64_t mask0 = mask0_of(k, NW);
    const uint64_t cap = idx->cap;
    Slot<NW> *table = (Slot<NW> *)idx->table;
    uint32_t *lists = nullptr, *cs_id = nullptr, *err = nullptr, *lpos = nullptr;
    uint64_t *off = nullptr, *cs_key = nullptr, *cs_rep = nullptr, *rep_of = nullptr;
    unsigned long long *cnt = nullptr;  // [0] n_kmers [1] bump [2] n_multi [3] n_cls [4] bump2
    pa::ErrOp op("index build");
    pa::Bufs b(st);
    PA_HIP(b.get(&off, cap * 8));
    PA_HIP(b.get(&cnt, 8 * 8));
    PA_HIP(b.get(&err, 4));
    // each window's place in its slot's genome list, taken in pass 1 (one-word
    // keys, plan::lpos_fits; PA_BUILD_LPOS=0: pass 2 takes the places by CAS,
    // as for keys of more than one word)
    {
        size_t fb = 0, tb = 0;
        const uint64_t total = idx->h_goff[G];  // (lpos is indexed by the concatenated position, as codes)
        if (NW == 1 && total > 0 && !env_is("PA_BUILD_LPOS", '0') && pa::dev_mem_info(&fb, &tb) == hipSuccess &&
            plan::lpos_fits(total, fb) && pa::dev_malloc_try((void **)&lpos, total * 4) != hipSuccess) {
            (void)hipGetLastError();
            lpos = nullptr;
        }
        b.adopt(lpos);
    }
    PA_HIP(hipMemsetAsync(cnt, 0, 8 * 8, st));
    PA_HIP(hipMemsetAsync(err, 0, 4, st));
    // pass 1 (one-word keys: a batch of windows per thread; wider keys one window at a time)
    for_each_genome_windows(idx, k, [&](uint32_t g, uint64_t start, uint64_t nwin) {
        const dim3 grid(grid_for((nwin + wpt - 1) / wpt));
        if constexpr (NW == 1)
            hipLaunchKernelGGL(k_build_insert1, grid, dim3(kBlock), 0, st, idx->codes, start, nwin, k, mask0, g, table,
                               idx->home, cnt + 0, err, wpt, lpos);
        else
            hipLaunchKernelGGL(k_build_insert<NW>, grid, dim3(kBlock), 0, st, idx->codes, start, nwin, k, mask0, g,
                               table, idx->home, cnt + 0, err, wpt);
    });
    PA_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_build_prep<NW>, dim3(scan_grid(cap)), dim3(kBlock), 0, st, table, cap, off, cnt + 1, cnt + 2,
                       lpos != nullptr ? 1 : 0);
    PA_HIP(hipGetLastError());
    unsigned long long h_cnt[8];
    uint32_t h_err = 0;
    PA_HIP(hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    if (h_err) {
        pa::set_error("index build: hash table overflow or insert livelock (internal error)");
        return PA_EINTERNAL;
    }
    idx->n_kmers = h_cnt[0];
    const uint64_t list_total = h_cnt[1], n_multi = h_cnt[2];
    idx->n_multi = 0;
    if (n_multi > 0) {
        PA_HIP(b.get(&lists, list_total * 4));
        for_each_genome_windows(idx, k, [&](uint32_t g, uint64_t start, uint64_t nwin) {
            const dim3 grid(grid_for((nwin + wpt - 1) / wpt));
            if constexpr (NW == 1)
                hipLaunchKernelGGL(k_build_fill1, grid, dim3(kBlock), 0, st, idx->codes, start, nwin, k, mask0, g, table,
                                   idx->home, G, off, lists, wpt, lpos);
            else
                hipLaunchKernelGGL(k_build_fill<NW>, grid, dim3(kBlock), 0, st, idx->codes, start, nwin, k, mask0, g,
                                   table, idx->home, G, off, lists, wpt);
        });
        PA_HIP(hipGetLastError());
        // distinct genome sets: a hash over the multi slots' genome lists.  A
        // reference has few distinct sets (C2: 342, 2000 genomes in families:
        // ~10^4) however many multi-genome k-mers (10^9 at 8 Gbp), so the hash
        // starts at 16 M entries and grows on overflow, up to 2 per k-mer
        const uint64_t cs_max = 2 * n_multi + 64;
        uint64_t cs_cap = std::min<uint64_t>(cs_max, (1ull << 24) + 64);
        unsigned sgrid = scan_grid(cap);
        int cache_pos = 0;
        for (;;) {
            PA_HIP(b.get(&cs_key, cs_cap * 8));
            PA_HIP(b.get(&cs_rep, cs_cap * 8));
            hipLaunchKernelGGL(k_fill_u64, dim3(scan_grid(cs_cap)), dim3(kBlock), 0,
                               st, cs_key, cs_cap, EMPTY);
            cache_pos = (uint64_t)G + cs_cap < 0xFFF00000ull ? 1 : 0;  // (G + position below pass 2's marks)
            hipLaunchKernelGGL(k_class_insert<NW>, dim3(sgrid), dim3(kBlock), 0, st, table, cap, G, off, lists,
                               cs_key, cs_rep, cs_cap, err, cache_pos);
            PA_HIP(hipGetLastError());
            PA_HIP(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, st));
            PA_HIP(hipStreamSynchronize(st));
            if (!(h_err & 4u) || cs_cap >= cs_max) break;
            b.free(cs_key);
            b.free(cs_rep);
            PA_HIP(hipMemsetAsync(err, 0, 4, st));
            cs_cap = std::min<uint64_t>(cs_max, 4 * cs_cap);
        }
        if (h_err & 4u) {
            pa::set_error("index build: genome-set table overflow (internal error)");
            return PA_EINTERNAL;
        }
        PA_HIP(b.get(&cs_id, cs_cap * 4));
        // class ids: at most min(n_multi, cs_cap) classes
        const uint64_t max_cls = std::min<uint64_t>(n_multi, cs_cap);
        PA_HIP(pa::dev_malloc(&idx->class_size, max_cls * 4));
        PA_HIP(pa::dev_malloc(&idx->class_off, max_cls * 8));
        PA_HIP(b.get(&rep_of, max_cls * 8));
        hipLaunchKernelGGL(k_class_number<NW>, dim3(scan_grid(cs_cap)), dim3(kBlock),
                           0, st, cs_key, cs_rep, cs_id, cs_cap, (const Slot<NW> *)table, idx->class_size,
                           idx->class_off, rep_of, cnt + 3, cnt + 4);
        PA_HIP(hipGetLastError());
        PA_HIP(hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
        const uint64_t n_cls = h_cnt[3], entries = h_cnt[4];
        if ((uint64_t)G + entries >= (uint64_t)PA_TILE_REP) {  // (bit 31 of a class id is the position bit, cls_of)
            pa::set_error("index build: too many distinct genome-set entries for 31-bit class ids");
            return PA_EUNSUPPORTED;
        }
        PA_HIP(pa::dev_malloc(&idx->class_genomes, std::max<uint64_t>(entries, 1) * 4));
        hipLaunchKernelGGL(k_class_copy, dim3((unsigned)std::min<uint64_t>(n_cls, 65536)), dim3(kBlock), 0, st, n_cls,
                           rep_of, idx->class_size, idx->class_off, off, lists, idx->class_genomes);
        if (G <= 64) {
            PA_HIP(pa::dev_malloc(&idx->class_mask, std::max<uint64_t>(entries, 1) * 8));
            hipLaunchKernelGGL(k_class_masks, dim3((unsigned)std::min<uint64_t>((n_cls + kBlock - 1) / kBlock, 4096)),
                               dim3(kBlock), 0, st, n_cls, idx->class_off, idx->class_genomes, idx->class_mask);
        }
        hipLaunchKernelGGL(k_class_assign<NW>, dim3(sgrid), dim3(kBlock), 0, st, table, cap, off, lists, cs_key,
                           cs_rep, cs_id, cs_cap, idx->class_size, idx->class_off, G, err, cache_pos);
        PA_HIP(hipGetLastError());
        PA_HIP(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
        if (h_err) {
            pa::set_error(h_err & 2 ? "index build: genome-set hash collision detected (refusing to merge sets)"
                                    : "index build: class table overflow (internal error)");
            return PA_EINTERNAL;
        }
        idx->n_multi = n_cls;
        idx->class_entries = entries;
        idx->device_bytes += n_cls * 12 + std::max<uint64_t>(entries, 1) * 4;
    }
    if (kTableOrdered && idx->n_kmers > 0) {
        if (idx->n_kmers >= cap) {  // (the sizing keeps the load <= 0.7: never)
            pa::set_error("index build: hash table full (internal error)");
            return PA_EINTERNAL;
        }
        hipLaunchKernelGGL(k_table_order<NW>, dim3(scan_grid(cap)), dim3(kBlock), 0, st,
                           table, idx->home);
        PA_HIP(hipGetLastError());
    }
    if (idx->tile_n > 0 && (uint64_t)G + idx->class_entries >= PA_TILE_REP) idx->tile_n = 0;  // ids need bit 31
    idx->tiles_pending = idx->tile_n > 0 ? 1 : 0;  // made by build_tiles_nw (index_prepare)
    return PA_OK;
}

// ---- step 7: the align-side view -------------------------------------------
// The genome tiling, flag planes and walk blocks, neighbour words and the
// Bloom filter (keys of one to three words, references whose genomes are each
// < 2^32 bases).  Made after the build scratch is freed -- at the end of
// pa_index_build, or deferred (PA_BUILD_DEFER_TILES) to pa_index_prepare / the
// first align call, so that an index used only for EXTSIM statistics
// (src/kmer.py:152-263) never pays for it.
// One function per part: it allocates, launches, sets its own fields of the
// index and adds its own device_bytes; what a failed one leaves behind goes
// with release_align_view.  The ORDER of the allocations and frees is part of
// the behaviour -- where a buffer lands in the slab pool has moved align speed
// by 10 % (plan::table_cap_distinct) -- so no part moves past another.

// f(int_c<NW>) for the key widths that have a tiling
template <class F>
auto with_tile_nw(int nw, F &&f) {
    return pa::with_int<3, 2, 1>(nw, f);
}

// The keys of the table into a Bloom filter of 2^lg words: the align-side one
// (bloom_word), or (nb) the neighbour-bit build's own (bloom_word_nb).
void bloom_fill(const pa_index *idx, hipStream_t st, uint64_t *bloom, uint32_t lg, bool nb) {
    const dim3 grid(scan_grid(idx->cap)), block(kBlock);
    if (idx->nw == 1 && nb)
        hipLaunchKernelGGL(k_bloom_build<true>, grid, block, 0, st, (const Slot<1> *)idx->table, idx->cap, bloom, lg,
                           (int)idx->k);
    else if (idx->nw == 1)
        hipLaunchKernelGGL(k_bloom_build<false>, grid, block, 0, st, (const Slot<1> *)idx->table, idx->cap, bloom, lg,
                           (int)idx->k);
    else if (idx->nw == 2)
        hipLaunchKernelGGL(k_bloom_build2<2>, grid, block, 0, st, (const Slot<2> *)idx->table, idx->cap, bloom, lg);
    else
        hipLaunchKernelGGL(k_bloom_build2<3>, grid, block, 0, st, (const Slot<3> *)idx->table, idx->cap, bloom, lg);
}

// The tiling itself: the genomes packed (tile_pk) and every window's class
// (tile_cls), every genome's chunks in one launch (k_tile_cls_all).
pa_status tile_classes(pa_index *idx, hipStream_t st) {
    const uint32_t G = idx->n_genomes;
    const int k = (int)idx->k, wpt = build_run();
    const uint64_t n = idx->tile_n, nwords = n / 32 + 32;  // padded: the walk reads up to 18 words past a position
    PA_HIP(pa::dev_malloc(&idx->tile_cls, n * 4));
    PA_HIP(pa::dev_malloc(&idx->tile_pk, nwords * 8));
    idx->device_bytes += n * 4 + nwords * 8;
    PA_HIP(hipMemsetAsync(idx->tile_cls, 0xFF, n * 4, st));
    hipLaunchKernelGGL(k_tile_pack, dim3(scan_grid(nwords)), dim3(kBlock), 0, st, idx->codes, n, idx->tile_pk, nwords);
    std::vector<uint64_t> ts(G + 1, 0);  // chunks before genome g
    for_each_genome_windows(idx, k, [&](uint32_t g, uint64_t, uint64_t nwin) { ts[g + 1] = (nwin + wpt - 1) / wpt; });
    for (uint32_t g = 0; g < G; g++) ts[g + 1] += ts[g];
    pa::Bufs b(st);
    uint64_t *d_ts = nullptr;
    PA_HIP(b.get(&d_ts, (G + 1) * 8));
    PA_HIP(hipMemcpyAsync(d_ts, ts.data(), (G + 1) * 8, hipMemcpyHostToDevice, st));
    if (ts[G] > 0) {
        with_tile_nw(idx->nw, [&](auto w) {
            hipLaunchKernelGGL(k_tile_cls_all<w()>, dim3(grid_for(ts[G])), dim3(kBlock), 0, st, idx->codes, idx->goff, d_ts,
                               G, k, mask0_of(k, w()), (Slot<w()> *)idx->table, idx->home, idx->tile_cls,
                               idx->class_genomes, idx->tpos_local, wpt);
        });
        PA_HIP(hipGetLastError());
    }
    return PA_OK;
}

// Below 2^33 bases: first occurrences as 33-bit concatenated positions
// (PA_TPOS_HI=0 keeps them genome-local: tests of that layout).
pa_status tile_first_concat(pa_index *idx, hipStream_t st) {
    if (!idx->tpos_local || idx->h_goff[idx->n_genomes] >= (1ull << 33) || env_is("PA_TPOS_HI", '0')) return PA_OK;
    with_tile_nw(idx->nw, [&](auto w) {
        hipLaunchKernelGGL(k_tpos_concat<w()>, dim3(scan_grid(idx->cap)), dim3(kBlock), 0, st,
                           (Slot<w()> *)idx->table, idx->cap, idx->n_genomes, idx->class_genomes, idx->goff);
    });
    PA_HIP(hipGetLastError());
    idx->tpos_local = 0;
    phase_mark("first occurrences concatenated");
    return PA_OK;
}

// The genome of every 2^16-th position (tile_gblk): genome_of is then one or two goff steps.
pa_status tile_genome_blocks(pa_index *idx, hipStream_t st) {
    const uint32_t G = idx->n_genomes;
    const uint64_t nb = (idx->tile_n >> 16) + 2;
    std::vector<uint32_t> gb(nb);
    for (uint64_t j = 0; j < nb; j++) {
        const uint64_t pos = j << 16;
        uint32_t g = (uint32_t)(std::upper_bound(idx->h_goff.begin(), idx->h_goff.begin() + G + 1, pos) -
                                idx->h_goff.begin());
        g = g == 0 ? 0 : g - 1;
        gb[j] = g >= G ? G - 1 : g;
    }
    PA_HIP(pa::dev_malloc(&idx->tile_gblk, nb * 4));
    idx->device_bytes += nb * 4;
    PA_HIP(hipMemcpyAsync(idx->tile_gblk, gb.data(), nb * 4, hipMemcpyHostToDevice, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

// The lane kernels' view: the repeat flags (k_tile_rep) and the walk blocks (tile_lw).
pa_status tile_walk_blocks(pa_index *idx, hipStream_t st) {
    const uint64_t n = idx->tile_n;
    const int k = (int)idx->k;
    with_tile_nw(idx->nw, [&](auto w) {
        hipLaunchKernelGGL(k_tile_rep<w()>, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 20)), dim3(256), 0,
                           st, idx->tile_pk, idx->tile_cls, n, k);
    });
    const uint64_t n_blocks = n / 64 + 8;  // padded: the 250-bp walk reads six blocks from any position
    PA_HIP(pa::dev_malloc(&idx->tile_lw, n_blocks * 32));
    hipLaunchKernelGGL(k_tile_walk, dim3((unsigned)std::min<uint64_t>((n_blocks + 3) / 4, 1u << 20)), dim3(256), 0, st,
                       idx->tile_cls, idx->tile_pk, n, idx->n_genomes, idx->tile_lw, n_blocks);
    idx->device_bytes += n_blocks * 32;
    phase_mark("repeats + walk blocks");
    return PA_OK;
}

// -- neighbour words (tile_nb): made once per index (C2: ~50 ms of kernels,
// ~0.12 s with the allocation) -- they repay themselves after ~4 reads per
// genome base.

// The device view of an index's neighbour words (wb: 8 or 4 bytes per word).
NbW nb_words(const pa_index *idx, uint64_t wb) {
    const uint64_t b0 = (uint64_t)(uintptr_t)idx->tile_nb;
    if (!idx->tile_nb1) return NbW{b0, 0, ~0ull};
    return NbW{b0, (uint64_t)(uintptr_t)idx->tile_nb1 - idx->nb_split * wb, idx->nb_split};
}

// The neighbour-bit build's Bloom filter of the keys (plan::nb_bloom_lg, in
// HBM, held by the caller's Bufs, which frees it): most of a window's 3k
// neighbours are absent and share its Bloom line (minimizer-chosen), so a
// probe costs an L2 hit instead of a table line.  nullptr when it does not fit
// (or, one-word keys, with PA_NB_BLOOM=0: A/B).
pa_status make_nb_bloom(pa_index *idx, hipStream_t st, pa::Bufs &b, uint64_t **out, uint32_t *out_lg) {
    *out = nullptr;
    *out_lg = 6;
    if ((idx->nw == 1 && env_is("PA_NB_BLOOM", '0')) || idx->n_kmers == 0) return PA_OK;
    size_t fb = 0, tb = 0;
    if (pa::dev_mem_info(&fb, &tb) != hipSuccess) fb = 0;
    const uint32_t lg = plan::nb_bloom_lg(idx->n_kmers, fb);
    uint64_t *bb = nullptr;
    if (lg == 0 || b.get(&bb, (1ull << lg) * 8) != hipSuccess) {
        (void)hipGetLastError();
        return PA_OK;
    }
    PA_HIP(hipMemsetAsync(bb, 0, (1ull << lg) * 8, st));
    if (idx->nw == 1)  // (the one-word build's phases are timed one by one)
        phase_mark(lg >= 30 ? "nb: Bloom alloc (lg >= 30)" : "nb: Bloom alloc (lg < 30)");
    bloom_fill(idx, st, bb, lg, true);
    PA_HIP(hipGetLastError());
    *out = bb;
    *out_lg = lg;
    return PA_OK;
}

// The two passes of one-word keys' neighbour words (k_nb_first, k_nb_copy):
// the forward words (rc = 0, full or present only) or tile_rcnb (rc = 1).
void nb_passes(const pa_index *idx, hipStream_t st, const NbW &words, int full, const uint64_t *bb, uint32_t bb_lg,
               int rc) {
    const uint64_t n = idx->tile_n;
    const Slot<1> *table = (const Slot<1> *)idx->table;
    hipLaunchKernelGGL(k_nb_first, dim3(scan_grid(n)), dim3(kBlock), 0, st, idx->tile_pk, idx->tile_cls, n, (int)idx->k,
                       table, idx->home, idx->n_genomes, words, full, idx->class_genomes, idx->goff, idx->tpos_local, bb,
                       bb_lg, rc);
    if (!rc) phase_mark("nb: first occurrences");
    hipLaunchKernelGGL(k_nb_copy, dim3(scan_grid(n)), dim3(kBlock), 0, st, idx->tile_pk, idx->tile_cls, n, (int)idx->k,
                       table, idx->home, idx->n_genomes, words, full, idx->class_genomes, idx->goff, idx->tpos_local);
    if (!rc) phase_mark("nb: copies");
}

// The reverse-complement neighbour bits (tile_rcnb, 12 B per base) when they
// leave a quarter of the free memory; bb: the build-time Bloom filter of the
// keys (nullable: every neighbour probed).
pa_status build_rcnb(pa_index *idx, hipStream_t st, const uint64_t *bb, uint32_t bb_lg) {
    const uint64_t n = idx->tile_n;
    idx->rcnb_pending = 0;
    size_t fr_b = 0, tr_b = 0;
    if (!(pa::dev_mem_info(&fr_b, &tr_b) == hipSuccess && plan::leaves_quarter(n * 12, fr_b) &&
          pa::dev_malloc(&idx->tile_rcnb, n * 12 + 64) == hipSuccess)) {
        (void)hipGetLastError();
        idx->tile_rcnb = nullptr;
        return PA_OK;  // (no room: the seedless reads are walked without them)
    }
    PA_HIP(hipMemsetAsync(idx->tile_rcnb, 0, n * 12 + 64, st));
    nb_passes(idx, st, NbW{(uint64_t)(uintptr_t)idx->tile_rcnb, 0, ~0ull}, 0, bb, bb_lg, 1);
    PA_HIP(hipGetLastError());
    idx->device_bytes += n * 12;
    phase_mark("nb: reverse complements");
    return PA_OK;
}

// Room for `words` neighbour words of wb bytes: one piece where the pool or
// the free device memory has room for it; else two pieces (plan::nb_split) --
// the first in the pool's largest free range, the second in the free device
// memory -- when both fit without giving idle slabs back; else one piece
// whatever it costs.  PA_NB_SPLIT=1 forces two halves (tests).
pa_status nb_alloc_words(pa_index *idx, uint64_t words, uint64_t wb) {
    const bool force_split = env_is("PA_NB_SPLIT", '1');
    if (!force_split && pa::dev_malloc_try(&idx->tile_nb, words * wb + 64) == hipSuccess) return PA_OK;
    (void)hipGetLastError();
    idx->tile_nb = nullptr;
    const plan::NbSplit sp = plan::nb_split(words, wb, pa::dev_pool_largest_free(), force_split);
    if (sp.usable) {
        if (pa::dev_malloc_try(&idx->tile_nb, sp.first * wb + 64) == hipSuccess &&
            pa::dev_malloc_try(&idx->tile_nb1, (words - sp.first) * wb + 64) == hipSuccess) {
            idx->nb_split = sp.first;
            return PA_OK;
        }
        (void)hipGetLastError();
        pa::dev_release(idx->tile_nb);
        pa::dev_release(idx->tile_nb1);
        idx->nb_split = ~0ull;
    }
    PA_HIP(pa::dev_malloc(&idx->tile_nb, words * wb + 64));
    return PA_OK;
}

// One-word keys: 3 words per base (plan::nb_word_bytes: present | specific,
// present only, or none), then the reverse-complement bits' turn.
pa_status build_nb1(pa_index *idx, hipStream_t st) {
    const uint64_t n = idx->tile_n, words = 3 * n;
    pa::Bufs b(st);
    size_t free_b = 0, total_b = 0;
    if (pa::dev_mem_info(&free_b, &total_b) != hipSuccess) return PA_OK;
    const uint64_t wb = plan::nb_word_bytes(n, free_b, env_is("PA_NB_HALF", '1'), idx->force_large != 0);
    if (wb == 0) return PA_OK;
    const int full = wb == 8 ? 1 : 0;
    PA_TRY(nb_alloc_words(idx, words, wb));
    phase_mark(idx->tile_nb1 ? "nb: alloc (two pieces)" : "nb: alloc");
    if (idx->tile_nb1) {
        PA_HIP(hipMemsetAsync(idx->tile_nb, 0, idx->nb_split * wb + 64, st));
        PA_HIP(hipMemsetAsync(idx->tile_nb1, 0, (words - idx->nb_split) * wb + 64, st));
    } else {
        PA_HIP(hipMemsetAsync(idx->tile_nb, 0, words * wb + 64, st));
    }
    phase_mark("nb: clear");
    uint64_t *bb = nullptr;
    uint32_t bb_lg = 6;
    PA_TRY(make_nb_bloom(idx, st, b, &bb, &bb_lg));
    phase_mark("nb: build Bloom");
    nb_passes(idx, st, nb_words(idx, wb), full, bb, bb_lg, 0);
    // the reverse-complement neighbour bits (tile_rcnb, 12 B per base):
    // only reads with no forward seed use them (k_align_lane_rc), so by
    // default they are left for the first align pass that queues enough
    // such reads (index_rcnb_wanted: C4's forward reads never do, and
    // its serving index skips their 0.35 s); PA_RCNB_EAGER=1 makes them
    // now, PA_NO_RCNB=1 never
    if (idx->k <= 31 && !env_is("PA_NO_RCNB", '1')) {
        if (env_is("PA_RCNB_EAGER", '1'))
            PA_TRY(build_rcnb(idx, st, bb, bb_lg));
        else
            idx->rcnb_pending = 1;
    }
    PA_HIP(b.free(bb));
    idx->nb_spec = full;
    idx->device_bytes += words * wb;
    return PA_OK;
}

// Two-word keys (k_nb_build2): 24 B per base (64-bit present words) when that
// leaves a quarter of the free memory; no reverse-complement bits.
pa_status build_nb2(pa_index *idx, hipStream_t st) {
    const uint64_t n = idx->tile_n;
    size_t free_b = 0, total_b = 0;
    if (pa::dev_mem_info(&free_b, &total_b) != hipSuccess || !plan::leaves_quarter(n * 24, free_b)) return PA_OK;
    PA_HIP(pa::dev_malloc(&idx->tile_nb, n * 24 + 64));
    PA_HIP(hipMemsetAsync(idx->tile_nb, 0, n * 24 + 64, st));
    pa::Bufs b(st);
    uint64_t *bb = nullptr;
    uint32_t bb_lg = 6;
    PA_TRY(make_nb_bloom(idx, st, b, &bb, &bb_lg));
    for (int pass = 0; pass < 2; pass++)
        hipLaunchKernelGGL(k_nb_build2, dim3(scan_grid(n)), dim3(kBlock), 0, st, idx->tile_pk, idx->tile_cls, n,
                           (int)idx->k, (const Slot<2> *)idx->table, idx->home, idx->n_genomes,
                           (unsigned long long *)idx->tile_nb, idx->class_genomes, idx->goff, idx->tpos_local, pass, bb,
                           bb_lg);
    PA_HIP(hipGetLastError());
    PA_HIP(b.free(bb));
    idx->nb_spec = 0;
    idx->device_bytes += n * 24;
    phase_mark("nb: two-word keys");
    return PA_OK;
}

// Three-word keys: neighbour summaries (k_nb_sum3), 0.5 B per base, in at most a quarter of the free memory.
pa_status build_nb3(pa_index *idx, hipStream_t st) {
    const uint64_t n = idx->tile_n, bytes = (n / 8 + 64) * 4;
    size_t free_b = 0, total_b = 0;
    if (pa::dev_mem_info(&free_b, &total_b) != hipSuccess || bytes > free_b / 4) return PA_OK;
    PA_HIP(pa::dev_malloc(&idx->tile_nb, bytes));
    PA_HIP(hipMemsetAsync(idx->tile_nb, 0, bytes, st));
    pa::Bufs b(st);
    uint64_t *bb = nullptr;
    uint32_t bb_lg = 6;
    PA_TRY(make_nb_bloom(idx, st, b, &bb, &bb_lg));
    hipLaunchKernelGGL(k_nb_sum3, dim3(scan_grid(n)), dim3(kBlock), 0, st, idx->tile_pk, idx->tile_cls, n, (int)idx->k,
                       (const Slot<3> *)idx->table, idx->home, (uint32_t *)idx->tile_nb, bb, bb_lg);
    PA_HIP(hipGetLastError());
    PA_HIP(b.free(bb));
    idx->nb_spec = 0;
    idx->device_bytes += bytes;
    phase_mark("nb: three-word summaries");
    return PA_OK;
}

// The neighbour words of the index's key width; PA_NO_NB=1: none (A/B, tests).
pa_status build_nb(pa_index *idx, hipStream_t st) {
    if (!env_is("PA_NO_NB", '1'))
        PA_TRY(idx->nw == 3 ? build_nb3(idx, st) : idx->nw == 2 ? build_nb2(idx, st) : build_nb1(idx, st));
    idx->nb_pending = 0;
    return PA_OK;
}

// The align-side Bloom filter of the keys (plan::align_bloom_lg_*: in the
// memory-side cache, else in HBM, else none).
pa_status tile_bloom(pa_index *idx, hipStream_t st) {
    plan::BloomSwitches sw;
    sw.mb_set = env("PA_BLOOM_MB") != nullptr;
    sw.mb = env_u64("PA_BLOOM_MB", 128);
    sw.hbm_off = env_is("PA_BLOOM_HBM", '0');
    sw.force_large = idx->force_large != 0;
    uint32_t lg = plan::align_bloom_lg_cache(idx->n_kmers, sw);
    size_t fb = 0, tb = 0;
    if (!lg && plan::align_bloom_hbm_wanted(idx->n_kmers, sw) && pa::dev_mem_info(&fb, &tb) == hipSuccess)
        lg = plan::align_bloom_lg_hbm(idx->n_kmers, fb);
    if (lg) {
        PA_HIP(pa::dev_malloc(&idx->bloom, (1ull << lg) * 8));
        PA_HIP(hipMemsetAsync(idx->bloom, 0, (1ull << lg) * 8, st));
        bloom_fill(idx, st, idx->bloom, lg, false);
        idx->bloom_lg = lg;
        idx->device_bytes += (1ull << lg) * 8;
    }
    phase_mark("Bloom");
    return PA_OK;
}

// The minimizer presence bitmap (one-word keys): 2^25 bits (4 MiB, the size of
// an XCD's L2) for references of up to ~30 M distinct minimizers (distinct
// k-mers / 9: a minimizer covers ~9 of a genome's k-mers), so that fewer than
// ~1 / 4 of the bits are set; none above (C4, C5) or with PA_NO_MM=1.
pa_status tile_minimizers(pa_index *idx, hipStream_t st) {
    const uint32_t lg = 25;
    if (idx->nw == 1 && !env_is("PA_NO_MM", '1') && idx->bloom && idx->n_kmers / 9 <= (1ull << lg) / 4 &&
        pa::dev_malloc(&idx->mm_bits, (1ull << lg) / 8) == hipSuccess) {
        PA_HIP(hipMemsetAsync(idx->mm_bits, 0, (1ull << lg) / 8, st));
        hipLaunchKernelGGL(k_mm_build, dim3(scan_grid(idx->cap)), dim3(kBlock), 0, st, (const Slot<1> *)idx->table,
                           idx->cap, idx->mm_bits, lg, (int)idx->k);
        idx->mm_lg = lg;
        idx->device_bytes += (1ull << lg) / 8;
    } else {
        idx->mm_bits = nullptr;
    }
    phase_mark("minimizer bitmap");
    return PA_OK;
}

// The reverse-complement plane (k_tile_rcp; one-word keys), 1 bit per base; PA_NO_RCP=1: none.
pa_status tile_rc_plane(pa_index *idx, hipStream_t st) {
    const uint64_t n_blocks = idx->tile_n / 64 + 5;  // padded like the walk blocks
    if (idx->nw == 1 && !env_is("PA_NO_RCP", '1') && pa::dev_malloc(&idx->tile_rcp, n_blocks * 8) == hipSuccess) {
        hipLaunchKernelGGL(k_tile_rcp, dim3((unsigned)std::min<uint64_t>((n_blocks + 3) / 4, 1u << 20)), dim3(256), 0, st,
                           idx->tile_cls, idx->tile_pk, idx->tile_n, (int)idx->k, (const Slot<1> *)idx->table, idx->home,
                           idx->bloom, idx->bloom_lg, idx->tile_rcp, n_blocks);
        idx->device_bytes += n_blocks * 8;
    } else {
        idx->tile_rcp = nullptr;
    }
    phase_mark("reverse-complement plane");
    return PA_OK;
}

// The parts in their order.  The tiling takes 6.5 B per base (class, flags,
// set sizes, 2-bit string): without that and a 2 GiB margin free there is none.
pa_status build_align_view(pa_index *idx, hipStream_t st) {
    size_t free_b = 0, total_b = 0;
    if (idx->tile_n > 0 &&
        (pa::dev_mem_info(&free_b, &total_b) != hipSuccess || idx->tile_n * 7 + (2ull << 30) > free_b))
        idx->tile_n = 0;
    if (idx->tile_n == 0) return PA_OK;
    PA_TRY(tile_classes(idx, st));
    phase_mark("tile classes");
    PA_TRY(tile_first_concat(idx, st));
    PA_TRY(tile_genome_blocks(idx, st));
    PA_TRY(tile_walk_blocks(idx, st));
    // one-substitution neighbours (build_nb): now, or -- when the caller
    // expects too few reads to repay them -- on the align that brings the
    // reads past that point (index_note_reads)
    if (idx->nb_skip)
        idx->nb_pending = 1;
    else
        PA_TRY(build_nb(idx, st));
    phase_mark("neighbour bits");
    PA_TRY(tile_bloom(idx, st));
    PA_TRY(tile_minimizers(idx, st));
    PA_TRY(tile_rc_plane(idx, st));
    PA_HIP(hipGetLastError());
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

template <int NW>
pa_status lookup_nw(const pa_index *idx, const uint8_t *d_kmers, uint64_t n, int64_t *d_cls, uint32_t *d_size,
                    hipStream_t st) {
    const int k = (int)idx->k;
    hipLaunchKernelGGL(k_lookup<NW>, dim3(grid_for(n)), dim3(kBlock), 0, st, (const Slot<NW> *)idx->table, idx->home,
                       d_kmers, n, k, mask0_of(k, NW), idx->n_genomes, idx->class_genomes, d_cls, d_size);
    PA_HIP(hipGetLastError());
    return PA_OK;
}

template <int NW>
void extsim_slots_nw(const pa_index *idx, const uint32_t *d_group, uint32_t n_groups, unsigned long long *total,
                     unsigned long long *uniq, unsigned long long *ccount, hipStream_t st) {
    int use_lds = n_groups <= 4096;
    size_t shm = use_lds ? (size_t)n_groups * 8 : 0;
    unsigned grid = grid_for(idx->cap) > 4096 ? 4096 : grid_for(idx->cap);
    hipLaunchKernelGGL(k_extsim_slots<NW>, dim3(grid), dim3(kBlock), shm, st, (const Slot<NW> *)idx->table, idx->cap,
                       idx->n_genomes, d_group, n_groups, total, uniq, ccount, use_lds);
}

}  // namespace

namespace pa {

// Everything an index owns on the device: the align-side view
// (release_align_view), the positions view, then the table, classes, codes and
// align scratch.  Every pointer is null afterwards: a second call frees nothing.
void index_release(pa_index *idx) {
    index_release_coverage(idx);
    release_align_view(idx);
    dev_release(idx->table);
    dev_release(idx->class_off);
    dev_release(idx->class_size);
    dev_release(idx->class_genomes);
    dev_release(idx->class_mask);
    dev_release(idx->codes);
    dev_release(idx->goff);
    dev_release(idx->fwd_len);
    dev_release(idx->ws.ptr);
    idx->ws.bytes = 0;
    dev_release(idx->queue);
    dev_release(idx->queue_hard);
    dev_release(idx->queue_na);
    dev_release(idx->queue_na2);
    dev_release(idx->queue_na_keys);
    dev_release(idx->queue_rc);
    dev_release(idx->queue_rc_anc);
    idx->queue_cap = 0;
    dev_release(idx->na_count);
    dev_release(idx->seg_cnt);
    dev_release(idx->qmask);
    dev_release(idx->qdrop);
    idx->qmask_cap = 0;
    dev_release(idx->counters);
    for (auto e : idx->ev_start) hipEventDestroy(e);
    for (auto e : idx->ev_stop) hipEventDestroy(e);
    for (auto &e : idx->kev) {
        hipEventDestroy(e.start);
        hipEventDestroy(e.stop);
    }
    idx->ev_start.clear();
    idx->ev_stop.clear();
    idx->kev.clear();
}

pa_status index_build_rcnb(pa_index *idx, hipStream_t st) {
    if (!idx->rcnb_pending) return PA_OK;
    TimedPhases tp(st);
    Bufs b(st);
    uint64_t *bb = nullptr;
    uint32_t bb_lg = 6;
    PA_TRY(make_nb_bloom(idx, st, b, &bb, &bb_lg));
    return build_rcnb(idx, st, bb, bb_lg);
}

pa_status index_note_reads(pa_index *idx, uint64_t n, hipStream_t st) {
    idx->reads_seen += n;
    if (!idx->nb_pending || !nb_repaid(idx->reads_seen, idx->tile_n, idx->nw)) return PA_OK;
    return build_nb(idx, st);
}

pa_status index_prepare(pa_index *idx, hipStream_t st, uint64_t reads_hint, bool complete) {
    if (!idx->tiles_pending) {  // (tiles made: the pending neighbour bits, if the reads still to come repay them)
        if (complete && idx->nb_pending &&
            (reads_hint == ~0ull || nb_repaid(idx->reads_seen + reads_hint, idx->tile_n, idx->nw))) {
            TimedPhases tp(st);
            return build_nb(idx, st);
        }
        return PA_OK;
    }
    idx->tiles_pending = 0;
    TimedPhases tp(st);  // (timed on its own unless a timed build called it)
    const uint64_t bases = idx->h_goff.empty() ? 0 : idx->h_goff.back();
    idx->nb_skip = reads_hint != ~0ull && !nb_repaid(reads_hint, bases, idx->nw);
    const pa_status rc = build_align_view(idx, st);
    idx->nb_skip = 0;
    if (rc != PA_OK) release_align_view(idx);  // the index stays usable without its align-side view
    return rc;
}

// The distinct k-mers of the encoded genomes, estimated (k_hll, plan::hll_distinct).
static pa_status estimate_distinct(pa_index *idx, hipStream_t st, uint64_t *distinct) {
    const int k = (int)idx->k;
    Bufs b(st);
    uint32_t *reg = nullptr;
    PA_HIP(b.get(&reg, (4ull << kHllBits)));
    PA_HIP(hipMemsetAsync(reg, 0, (4ull << kHllBits), st));
    for_each_genome_windows(idx, k, [&](uint32_t, uint64_t start, uint64_t nwin) {
        const dim3 grid(grid_for((nwin + kRun - 1) / kRun));
        with_nw(idx->nw, [&](auto w) {
            hipLaunchKernelGGL(k_hll<w()>, grid, dim3(kBlock), 0, st, idx->codes, start, nwin, k, mask0_of(k, w()), reg);
        });
    });
    std::vector<uint32_t> h(1u << kHllBits);
    PA_HIP(hipMemcpyAsync(h.data(), reg, (4ull << kHllBits), hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    *distinct = plan::hll_distinct(h.data(), (uint32_t)h.size());
    return PA_OK;
}

// The table's capacity by the plan (pa_index_plan.h): on the genome windows,
// else -- or when PA_CAP_HLL=1 or the large layout ask for it (tests, A/B) --
// on the distinct estimate.
static pa_status table_capacity(pa_index *idx, uint64_t windows, hipStream_t st, uint64_t *out) {
    const int sb = slot_bytes(idx->nw);
    size_t free_b = 0, total_b = 0;
    PA_HIP(pa::dev_mem_info(&free_b, &total_b));
    uint64_t cap = plan::table_cap_windows(windows, sb, free_b, idx->compact_table && idx->nw == 1,
                                           env_int("PA_CAP_MULT", plan::kNoCapMult));
    const bool forced = env_is("PA_CAP_HLL", '1') || idx->force_large || free_b == 0;
    if (forced) cap = 0;
    if (cap == 0 && idx->k > 0 && windows > 0) {
        uint64_t distinct = 0;
        PA_TRY(estimate_distinct(idx, st, &distinct));
        idx->distinct_estimate = distinct;
        if (forced) PA_HIP(pa::dev_mem_info(&free_b, &total_b));
        const char *first = env("PA_CAP_DISTINCT");  // A/B: this many slots per distinct k-mer first
        cap = plan::table_cap_distinct(distinct, windows, sb, free_b, forced, first ? std::atof(first) : 0.0);
        if (cap == 0) {
            set_error("index build: the k-mer table of ~" + std::to_string(distinct) +
                      " distinct k-mers does not fit the free device memory" +
                      (idx->both_strands ? " (a both-strand index needs about twice a forward index's memory)" : ""));
            return PA_ENOMEM;
        }
    }
    *out = plan::table_cap_lines(cap);
    return PA_OK;
}

pa_status index_build(pa_index *idx, const char *genomes, const uint64_t *goff, uint32_t n, int64_t k,
                      hipStream_t st, bool defer_tiles, uint8_t *dev_codes) {
    TimedPhases tm(st);
    idx->k = k;
    idx->nw = k > 0 ? key_words(k) : 1;
    idx->n_genomes = n;
    // Both strands: the index is the forward index of the regions T(g) = g + N +
    // reverse complement(g) -- everything below (sizing included) sees those
    // regions as its genomes; the caller's text and offsets are forward only.
    // (dev_codes, index_reduce: goff already describes the gathered regions.)
    const bool both = idx->both_strands != 0;
    const uint64_t text_off = goff[0], fwd_total = goff[n] - goff[0];  // the caller's text
    std::vector<uint64_t> fwd_goff, region_goff;
    if (both) {
        idx->h_fwd_len.resize(n);
        for (uint32_t g = 0; g < n; g++) {
            const uint64_t len = goff[g + 1] - goff[g];
            idx->h_fwd_len[g] = dev_codes ? (len ? (len - 1) / 2 : 0) : len;
        }
        if (!dev_codes) {
            fwd_goff.assign(goff, goff + n + 1);
            for (auto &o : fwd_goff) o -= goff[0];
            region_goff.assign(n + 1, 0);
            for (uint32_t g = 0; g < n; g++) region_goff[g + 1] = region_goff[g] + strand_region(idx->h_fwd_len[g]);
            goff = region_goff.data();
        }
    }
    idx->h_goff.assign(goff, goff + n + 1);
    const uint64_t total = goff[n] - goff[0];
    uint64_t windows = 0;
    for (uint32_t g = 0; g < n; g++) {
        uint64_t len = goff[g + 1] - goff[g];
        if (both) {  // (the windows across the join hold its N: they are counted on each strand only)
            len = idx->h_fwd_len[g];
            if (k > 0 && (uint64_t)k <= len) windows += 2 * (len - (uint64_t)k + 1);
            continue;
        }
        if (k > 0 && (uint64_t)k <= len) windows += len - (uint64_t)k + 1;
    }
    for (auto &o : idx->h_goff) o -= goff[0];
    idx->total_windows = windows;
    // genome tiling for keys of one or two words (k <= 63) while positions fit 32 bits (tpos);
    // PA_NO_TILE=1 turns it off (A/B measurements)
    uint64_t max_glen = 0;
    for (uint32_t g = 0; g < n; g++) max_glen = std::max<uint64_t>(max_glen, goff[g + 1] - goff[g]);
    idx->tile_n = (idx->nw <= 3 && k > 0 && total > 0 && max_glen < 0xFFFFFFFFull && !env_is("PA_NO_TILE", '1'))
                      ? total : 0;
    idx->tpos_local = total >= 0xFFFFFFFFull ? 1 : 0;
    // PA_LAYOUT=large (tests): every choice the build makes for a reference too
    // large for the default layout (C5: 8 Gbp) -- table sized on the distinct
    // estimate at 1.43 slots per k-mer, genome-local first occurrences, the 12-B
    // present-only neighbour bits, no Bloom filter -- on a small reference
    if (const char *e = env("PA_LAYOUT")) idx->force_large = std::strcmp(e, "large") == 0;
    idx->tpos_local |= env_is("PA_TPOS_LOCAL", '1');  // tests: the >= 4 Gbp layout
    idx->tpos_local |= idx->force_large;
    if (dev_codes)
        idx->codes = dev_codes;  // (index_reduce: the 2-bit codes are on the device already)
    else
        PA_HIP(pa::dev_malloc(&idx->codes, std::max<uint64_t>(total, 1)));
    PA_HIP(pa::dev_malloc(&idx->goff, (n + 1) * 8));
    PA_HIP(pa::dev_malloc(&idx->counters, 40 * 8));
    PA_HIP(hipMemsetAsync(idx->counters, 0, 40 * 8, st));
    PA_HIP(hipMemcpyAsync(idx->goff, idx->h_goff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (both) {
        PA_HIP(pa::dev_malloc(&idx->fwd_len, std::max<uint64_t>(n, 1) * 8));
        PA_HIP(hipMemcpyAsync(idx->fwd_len, idx->h_fwd_len.data(), (uint64_t)n * 8, hipMemcpyHostToDevice, st));
    }
    if (total > 0 && !dev_codes) {
        // step 1: the forward text is uploaded and encoded (both strands: k_encode_strands writes the regions)
        uint8_t *ascii = nullptr;
        uint64_t *d_fgoff = nullptr;
        unsigned long long *bad = nullptr, h_bad = ~0ull;
        Bufs b(st);  // (the staging buffers go before the table is allocated)
        PA_HIP(b.get(&ascii, both ? fwd_total + kExpandPad : fwd_total));
        if (both) PA_HIP(b.get(&d_fgoff, (n + 1) * 8));
        PA_HIP(b.get(&bad, 8));
        tm.mark("alloc");
        PA_HIP(hipMemsetAsync(bad, 0xFF, 8, st));
        if (both) PA_HIP(hipMemcpyAsync(d_fgoff, fwd_goff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
        PA_HIP(hipMemcpyAsync(ascii, genomes + text_off, fwd_total, hipMemcpyHostToDevice, st));
        tm.mark("upload");
        if (both)
            hipLaunchKernelGGL(k_encode_strands, dim3(scan_grid((total + kExpandRun - 1) / kExpandRun)), dim3(kBlock), 0,
                               st, ascii, d_fgoff, idx->goff, n, idx->codes, bad);
        else
            hipLaunchKernelGGL(k_encode, dim3(scan_grid(total)), dim3(kBlock), 0, st, ascii, idx->codes, total, bad);
        PA_HIP(hipMemcpyAsync(&h_bad, bad, 8, hipMemcpyDeviceToHost, st));
        PA_HIP(hipStreamSynchronize(st));
        if (h_bad != ~0ull) {
            set_error("genome text may only contain A, C, G, T and N (byte " + std::to_string(h_bad) + ")");
            return PA_EINVAL;
        }
    }
    tm.mark("encode");
    // step 2: the table
    const int sb = slot_bytes(idx->nw);
    uint64_t cap = 0;
    PA_TRY(table_capacity(idx, windows, st, &cap));
    idx->cap = cap;
    idx->home = pad::HomeCfg{cap};
    PA_HIP(pa::dev_malloc(&idx->table, idx->cap * sb));
    PA_HIP(hipMemsetAsync(idx->table, 0xFF, idx->cap * sb, st));
    idx->device_bytes = idx->cap * sb + total + (n + 1) * 8 + (both ? (uint64_t)n * 8 : 0);
    tm.mark("table");
    if (k <= 0 || windows == 0) return PA_OK;
    pa_status rc = PA_EUNSUPPORTED;
    if (idx->nw >= 1 && idx->nw <= 8)
        rc = with_nw(idx->nw, [&](auto w) { return build_nw<w()>(idx, st); });
    else
        set_error("unsupported k");
    tm.mark("insert + sets");
    if (rc != PA_OK || defer_tiles) return rc;
    rc = index_prepare(idx, st);
    tm.mark("tiles");
    return rc;
}

// The index of some of its genomes, in place: their 2-bit codes gathered on
// the device (one copy per run of consecutive kept genomes), everything else
// released, then the build from those codes.  The EXTSIM rebuild
// (KmerReference._filter_similar_genomes; the reference prunes its dict,
// src/kmer.py:232-263) without concatenating and uploading the kept genomes
// again: C5's 1200 of 2000 genomes, 4.8 GB.
// The kept genomes' codes are gathered into a fresh buffer while the old index
// is still whole (an error leaves it usable); when that buffer does not fit
// beside the old index, they are compacted inside the old codes buffer instead
// (sel ascending: every run moves towards the front), through a small bounce
// buffer where a run's source and destination overlap, so the peak is never
// above the old index.
pa_status index_reduce(pa_index *idx, const uint32_t *sel, uint32_t n, hipStream_t st, bool defer_tiles) {
    std::vector<uint64_t> goff(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) goff[i + 1] = goff[i] + (idx->h_goff[sel[i] + 1] - idx->h_goff[sel[i]]);
    // runs of consecutive kept genomes: (destination, source, length)
    struct Run {
        uint64_t to, from, len;
    };
    std::vector<Run> runs;
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i;
        while (j + 1 < n && sel[j + 1] == sel[j] + 1) j++;
        const uint64_t from = idx->h_goff[sel[i]], len = idx->h_goff[sel[j] + 1] - from;
        if (len) runs.push_back({goff[i], from, len});
        i = j + 1;
    }
    const int64_t k = idx->k;
    const int device = idx->device;
    const bool profile = idx->profile;  // (set through the C ABI: kept across the rebuild)
    const int compact = idx->compact_table;  // (pa_index_reduce's flags)
    const int both = idx->both_strands;      // (fixed at the build: whole regions are gathered, so it is kept)
    // pa.h: on failure the index holds nothing and may only be freed -- so a
    // failed copy never leaves half-compacted codes behind a valid-looking index
    auto empty_index = [&]() {
        index_release(idx);
        *idx = pa_index();
        idx->device = device;
        idx->profile = profile;
        idx->compact_table = compact;
        idx->both_strands = both;
    };
    auto fail = [&](hipError_t err, uint8_t *scratch) -> pa_status {
        (void)hipStreamSynchronize(st);  // (the queued copies may still read or write scratch)
        pa::dev_free(scratch);
        empty_index();
        idx->released = 1;
        set_error(std::string("index reduce: ") + hipGetErrorString(err) + " (the index was released)");
        return err == hipErrorOutOfMemory ? PA_ENOMEM : PA_EDEVICE;
    };
    uint8_t *codes = nullptr;
    hipError_t e = pa::dev_malloc(&codes, std::max<uint64_t>(goff[n], 1));
    if (e == hipSuccess && env_is("PA_REDUCE_INPLACE", '1')) {  // tests: force the in-place path
        pa::dev_free(codes);
        codes = nullptr;
        e = hipErrorOutOfMemory;
    }
    if (e == hipSuccess) {
        for (size_t r = 0; r < runs.size() && e == hipSuccess; r++)
            e = hipMemcpyAsync(codes + runs[r].to, idx->codes + runs[r].from, runs[r].len, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(e, codes);
    } else if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        codes = idx->codes;
        constexpr uint64_t kBounce = 64ull << 20;
        // the bounce buffer, if any run overlaps its destination, is taken
        // before the first copy: a failure here changes nothing yet
        uint8_t *bounce = nullptr;
        bool overlap = false;
        for (const Run &u : runs) overlap |= u.to != u.from && u.to + u.len > u.from;
        // PA_REDUCE_INJECT=bounce|copy (tests): the bounce allocation, or the
        // copy after the first run, fails
        const char *inj = env("PA_REDUCE_INJECT");
        const bool inj_bounce = inj && std::strcmp(inj, "bounce") == 0, inj_copy = inj && std::strcmp(inj, "copy") == 0;
        if (overlap && (e = inj_bounce ? hipErrorOutOfMemory : pa::dev_malloc(&bounce, kBounce)) != hipSuccess) {
            (void)hipGetLastError();
            set_error(std::string("index reduce: ") + hipGetErrorString(e) + " (the index is unchanged)");
            return e == hipErrorOutOfMemory ? PA_ENOMEM : PA_EDEVICE;
        }
        e = hipSuccess;
        for (size_t r = 0; r < runs.size() && e == hipSuccess; r++) {
            const Run &u = runs[r];
            if (u.to == u.from) continue;
            if (u.to + u.len <= u.from) {  // no overlap: one copy
                e = hipMemcpyAsync(codes + u.to, codes + u.from, u.len, hipMemcpyDeviceToDevice, st);
                continue;
            }
            for (uint64_t o = 0; o < u.len && e == hipSuccess; o += kBounce) {  // front to back: a chunk's source is read before it is overwritten
                const uint64_t c = std::min(kBounce, u.len - o);
                e = hipMemcpyAsync(bounce, codes + u.from + o, c, hipMemcpyDeviceToDevice, st);
                if (e == hipSuccess) e = hipMemcpyAsync(codes + u.to + o, bounce, c, hipMemcpyDeviceToDevice, st);
            }
            if (inj_copy && e == hipSuccess) e = hipErrorOutOfMemory;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(e, bounce);  // (codes are the index's own: released with it)
        pa::dev_free(bounce);
        idx->codes = nullptr;  // (kept: the rebuild's codes)
    } else {
        PA_HIP(e);
    }
    empty_index();
    const pa_status rc = index_build(idx, nullptr, goff.data(), n, k, st, defer_tiles, codes);
    if (rc != PA_OK) {  // (the error text stays: releasing sets none)
        empty_index();
        idx->released = 1;
    }
    return rc;
}

pa_status index_lookup(const pa_index *idx, const char *kmers, uint64_t n, uint32_t kmer_len, int64_t *cls_out,
                       uint32_t *size_out, hipStream_t st) {
    if (n == 0) return PA_OK;
    if ((int64_t)kmer_len != idx->k || idx->k <= 0 || idx->n_kmers == 0) {
        for (uint64_t i = 0; i < n; i++) {
            cls_out[i] = -1;
            if (size_out) size_out[i] = 0;
        }
        return PA_OK;
    }
    uint8_t *d_k = nullptr;
    int64_t *d_c = nullptr;
    uint32_t *d_s = nullptr;
    Bufs b(st);
    PA_HIP(b.get(&d_k, n * kmer_len));
    PA_HIP(b.get(&d_c, n * 8));
    PA_HIP(b.get(&d_s, n * 4));
    PA_HIP(hipMemcpyAsync(d_k, kmers, n * kmer_len, hipMemcpyHostToDevice, st));
    PA_TRY(with_nw(idx->nw, [&](auto w) { return lookup_nw<w()>(idx, d_k, n, d_c, d_s, st); }));
    PA_HIP(hipMemcpyAsync(cls_out, d_c, n * 8, hipMemcpyDeviceToHost, st));
    if (size_out) PA_HIP(hipMemcpyAsync(size_out, d_s, n * 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

pa_status index_extsim_stats(const pa_index *idx, const uint32_t *group_of, uint32_t n_groups, uint64_t *total,
                             uint64_t *uniq, uint64_t *inter, hipStream_t st) {
    const uint64_t ng2 = (uint64_t)n_groups * n_groups;
    for (uint32_t i = 0; i < n_groups; i++) total[i] = uniq[i] = 0;
    for (uint64_t i = 0; i < ng2; i++) inter[i] = 0;
    if (idx->n_kmers == 0 || n_groups == 0) return PA_OK;
    uint32_t *d_group = nullptr, *scratch = nullptr;
    unsigned long long *d_tot = nullptr, *d_uniq = nullptr, *d_inter = nullptr, *d_cc = nullptr;
    const uint64_t nm = std::max<uint64_t>(idx->n_multi, 1);
    const uint64_t n_rec = std::max<uint64_t>(idx->class_entries, 1);
    const unsigned cgrid = (unsigned)std::min<uint64_t>(nm, 1024);
    Bufs b(st);
    PA_HIP(b.get(&d_group, (uint64_t)idx->n_genomes * 4));
    PA_HIP(b.get(&d_tot, n_groups * 8));
    PA_HIP(b.get(&d_uniq, n_groups * 8));
    PA_HIP(b.get(&d_inter, ng2 * 8));
    PA_HIP(b.get(&d_cc, n_rec * 8));
    PA_HIP(b.get(&scratch, (uint64_t)cgrid * (idx->n_genomes + 1) * 4));
    PA_HIP(hipMemcpyAsync(d_group, group_of, (uint64_t)idx->n_genomes * 4, hipMemcpyHostToDevice, st));
    PA_HIP(hipMemsetAsync(d_tot, 0, n_groups * 8, st));
    PA_HIP(hipMemsetAsync(d_uniq, 0, n_groups * 8, st));
    PA_HIP(hipMemsetAsync(d_inter, 0, ng2 * 8, st));
    PA_HIP(hipMemsetAsync(d_cc, 0, n_rec * 8, st));
    with_nw(idx->nw, [&](auto w) { extsim_slots_nw<w()>(idx, d_group, n_groups, d_tot, d_uniq, d_cc, st); });
    if (idx->n_multi > 0)
        hipLaunchKernelGGL(k_extsim_classes, dim3(cgrid), dim3(kBlock), 0, st, idx->n_multi, idx->class_off,
                           idx->class_size, idx->class_genomes, d_group, n_groups, d_cc, d_tot, d_inter, scratch,
                           (uint64_t)idx->n_genomes + 1);
    PA_HIP(hipGetLastError());
    PA_HIP(hipMemcpyAsync(total, d_tot, n_groups * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(uniq, d_uniq, n_groups * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(inter, d_inter, ng2 * 8, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

pa_status reads_synthesize(const pa_index *idx, pa_reads *r, uint64_t n, uint32_t len, uint64_t first,
                           uint64_t seed, double sub_rate, double rc_rate, double foreign_rate, hipStream_t st) {
    std::vector<uint32_t> elig;
    const std::vector<uint64_t> flen = forward_lengths(idx);
    for (uint32_t g = 0; g < idx->n_genomes; g++)
        if (flen[g] >= len) elig.push_back(g);
    if (elig.empty()) {
        set_error("pa_reads_synthesize: no genome is at least read_len long");
        return PA_EINVAL;
    }
    r->device = idx->device;
    r->n = n;
    r->n_bases = n * len;
    r->max_len = len;
    Bufs b(st);
    uint32_t *d_elig = nullptr;
    PA_HIP(pa::dev_malloc(&r->seq, r->n_bases + kReadPad));  // (r's: the caller frees them with it)
    PA_HIP(pa::dev_malloc(&r->qual, r->n_bases + kReadPad));
    PA_HIP(pa::dev_malloc(&r->off, (n + 1) * 8));
    PA_HIP(b.get(&d_elig, elig.size() * 4));
    PA_HIP(hipMemcpyAsync(d_elig, elig.data(), elig.size() * 4, hipMemcpyHostToDevice, st));
    if (n == 0 || len == 0) {
        PA_HIP(hipMemsetAsync(r->off, 0, (n + 1) * 8, st));
    } else {
        auto th = [](double x) {
            const double t = x < 0 ? 0 : (x > 1 ? 1 : x);
            return (uint32_t)std::min(16777215.0, t * 16777216.0);
        };
        hipLaunchKernelGGL(k_synth_reads, dim3(scan_grid(r->n_bases)),
                           dim3(kBlock), 0, st, idx->codes, idx->goff, d_elig, (uint32_t)elig.size(), n, len, first,
                           seed, th(sub_rate), th(rc_rate), th(foreign_rate), r->seq, r->qual, r->off, idx->fwd_len);
    }
    PA_HIP(hipGetLastError());
    PA_HIP(hipStreamSynchronize(st));
    return PA_OK;
}

}  // namespace pa

namespace {
__global__ void k_warm_index() {}
}  // namespace

namespace pa {
// Loads this file's code object (a first launch from a module loads it): the
// CLI's runtime-start thread calls it so that the load overlaps host work.
void warm_index(hipStream_t st) { hipLaunchKernelGGL(k_warm_index, dim3(1), dim3(64), 0, st); }
}  // namespace pa
