// The index build's sizing decisions (pa_index.hip) as pure functions: integer
// arithmetic on (windows, distinct k-mers, free bytes, flags).  Host only: no
// HIP, no environment, no allocation -- the caller reads the switches and the
// free memory and passes them in, so that the sizes that matter (C5: 8 Gbp in
// 288 GB) are reached by a test without a device (tests/host/index_plan_main.cpp).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>

namespace pa {
namespace plan {

// ---- the k-mer table ------------------------------------------------------
// Table capacity (whole 64-B lines).  Load 1/4 of the genome windows when
// the table fits a third of the free device memory (absent keys -- the
// sequencing-error windows -- then end in their home slot 3 times out of
// 4), else 1/2 of the windows if table + build scratch fit; a reference
// too large for either is sized on its distinct k-mers (HyperLogLog
// estimate + 3 %): 4, 2.5, 2 or 1.43 slots per distinct k-mer, the largest that
// fits.  The build needs 8 B of scratch per slot (list offsets; the rest
// of its bookkeeping lives in the slots) and at most 4 B per genome window
// for the genome lists; the sizing still counts 20 B per slot, which
// leaves the align-side view (tiles, neighbour bits) its room.
inline bool table_fits(uint64_t cap, int slot_bytes, uint64_t windows, uint64_t free_b) {
    const uint64_t per_slot = (uint64_t)slot_bytes + 20, reserve = windows * 4 + (1ull << 30);
    return cap * per_slot + reserve <= free_b;
}

constexpr int kNoCapMult = INT_MIN;  // cap_mult: PA_CAP_MULT not set

// The first stage, on the genome windows: 4 or 2 slots per window, or 0 when
// neither fits (the distinct estimate then decides, table_cap_distinct).
// compact (PA_BUILD_COMPACT, one-word keys: the caller checks the width): 2 per
// window -- the scans of the table and its first touches shrink with it;
// aligns ~2-4 % slower, C4 job +13 %, C2 +15 %; two- and three-word keys,
// inserted one window at a time, built slower at that load: k = 63 0.171 ->
// 0.196 s.  cap_mult (PA_CAP_MULT): that many slots per window, at least 2,
// whatever fits.
inline uint64_t table_cap_windows(uint64_t windows, int slot_bytes, uint64_t free_b, bool compact,
                                  int cap_mult = kNoCapMult) {
    uint64_t cap = 0;
    if (!compact && (4 * windows + 64) * (uint64_t)slot_bytes <= free_b / 3 &&
        table_fits(4 * windows + 64, slot_bytes, windows, free_b))
        cap = 4 * windows + 64;
    else if (table_fits(2 * windows + 64, slot_bytes, windows, free_b))
        cap = 2 * windows + 64;
    if (cap_mult != kNoCapMult) cap = (uint64_t)std::max(2, cap_mult) * windows + 64;
    return cap;
}

// The second stage, on the distinct estimate: the first multiplier that fits,
// 0 when none does (PA_ENOMEM).  forced (PA_CAP_HLL=1, PA_LAYOUT=large: this
// stage on a reference the first would have served) never takes a multiplier
// above 1.5.  first_mult (PA_CAP_DISTINCT, A/B): within [1.2, 8] it is tried
// first, then 2 and 1.43; any other value (0: unset) changes nothing.
// (2.5 before 2: C5's kept 2.65 G k-mers at load 0.39 instead of 0.48 run 4-7 % faster,
// profiles/r05/ab_c5_table.txt -- and build ~1.5 s slower: the larger table leaves the
// neighbour words no free range in the slab pool, whose trim then stalls a hipMalloc)
// (PA_BUILD_COMPACT does not apply here: C5's job index at 2 per k-mer
// built no faster, 4.58 vs 4.47 s, and the serving index built after
// it in the same process, placed in its freed slabs, aligned 10 % slower)
inline uint64_t table_cap_distinct(uint64_t distinct, uint64_t windows, int slot_bytes, uint64_t free_b, bool forced,
                                   double first_mult = 0.0) {
    double mults[4] = {4.0, 2.5, 2.0, 1.43};
    if (first_mult >= 1.2 && first_mult <= 8.0) mults[0] = first_mult, mults[1] = 2.0, mults[2] = 1.43;
    for (double mult : mults) {
        const uint64_t c = (uint64_t)(mult * (double)distinct) + 64;
        if (forced && mult > 1.5) continue;
        if (table_fits(c, slot_bytes, windows, free_b)) return c;
    }
    return 0;
}

// Whole 64-B lines (the fast kernel probes a line per step); an empty index keeps 64 slots.
inline uint64_t table_cap_lines(uint64_t cap) { return ((cap ? cap : 64) + 3) / 4 * 4; }

// The distinct k-mers of a HyperLogLog register file (k_hll: reg[i] = the
// largest rank seen by register i, 0: none): the raw estimate alpha m^2 / sum
// 2^-reg, below 2.5 m with empty registers the small-range correction m ln(m /
// empty); + 3 % (the estimator's error at 2^16 registers is ~0.4 %) + 64.
inline uint64_t hll_distinct(const uint32_t *reg, uint32_t n_reg) {
    const double mm = (double)n_reg;
    double z = 0;
    uint32_t zeros = 0;
    for (uint32_t i = 0; i < n_reg; i++) {
        z += std::ldexp(1.0, -(int)reg[i]);
        zeros += reg[i] == 0;
    }
    double est = (0.7213 / (1.0 + 1.079 / mm)) * mm * mm / z;
    if (est < 2.5 * mm && zeros) est = mm * std::log(mm / zeros);
    return (uint64_t)(est * 1.03) + 64;
}

// Pass 1's per-window list places (lpos): 4 B per base, while that fits an
// eighth of the free memory.
inline bool lpos_fits(uint64_t bases, uint64_t free_b) { return bases * 4 <= free_b / 8; }

// ---- Bloom filters (2^lg 64-bit words; bloom_block: lg <= 33) --------------
// The neighbour-bit build's filter of the keys: ~16 bits per key (4 * 2^lg >=
// n_kmers words), shrunk to a quarter of the free memory, accepted at 8 bits
// per key or more.  0: none (no keys, or no room).
inline uint32_t nb_bloom_lg(uint64_t n_kmers, uint64_t free_b) {
    if (n_kmers == 0) return 0;
    uint32_t lg = 6;
    while (lg < 33 && (1ull << lg) * 4 < n_kmers) lg++;
    while (lg > 6 && (1ull << lg) * 8 > free_b / 4) lg--;
    return (1ull << lg) * 64 < n_kmers * 8 ? 0 : lg;
}

// The align-side filter, for the lane kernel's probes of windows off the walk
// (almost all absent).  In the memory-side cache: 16 bits per key up to
// PA_BLOOM_MB (default 128: with minimizer blocks of 16 B a run of ~9 keys
// shares one block, so the filter needs the room -- at 64 MB c2rc's
// k_align_lane_na took 3.78 ms, at 128 MB 3.24; 0: none), fewer down to 8 bits
// per key.  A reference too large for that gets one in HBM, 16 (down to 8)
// bits per key in at most 1/8 of the free memory (PA_BLOOM_HBM=0: none): the
// off-walk windows of a read cluster around its mismatches and share
// minimizer lines, so one Bloom line answers several table lines (C4 2.94 ->
// 3.30, C5 2.32 -> 2.70 G reads/s; C2 keeps the cache-sized one: 3.49 vs 3.41
// with 134 MB).  The large-reference layout (PA_LAYOUT=large) takes the HBM
// form.
struct BloomSwitches {
    bool mb_set = false;   // PA_BLOOM_MB given
    uint64_t mb = 128;     //   its value
    bool hbm_off = false;  // PA_BLOOM_HBM=0
    bool force_large = false;
};
inline uint32_t bloom_lg16(uint64_t n_kmers) {  // 16 bits per key
    uint32_t lg = 6;
    while (lg < 33 && (1ull << lg) * 64 < n_kmers * 16) lg++;
    return lg;
}
// the cache-sized form: its lg, 0 when it does not serve
inline uint32_t align_bloom_lg_cache(uint64_t n_kmers, const BloomSwitches &s) {
    const uint64_t cap_b = s.force_large ? 0ull : (s.mb_set ? s.mb : 128ull) << 20;
    uint32_t lg = bloom_lg16(n_kmers);
    while (lg > 6 && (1ull << lg) * 8 > cap_b) lg--;
    const bool ok = cap_b > 0 && n_kmers > 0 && (1ull << lg) * 64 >= n_kmers * 8 && (1ull << lg) * 8 <= cap_b;
    return ok ? lg : 0;
}
// whether the HBM form is tried after it (a given PA_BLOOM_MB means the cache-sized one or none)
inline bool align_bloom_hbm_wanted(uint64_t n_kmers, const BloomSwitches &s) {
    return n_kmers > 0 && !s.hbm_off && (!s.mb_set || s.force_large);
}
inline uint32_t align_bloom_lg_hbm(uint64_t n_kmers, uint64_t free_b) {
    uint32_t lg = bloom_lg16(n_kmers);
    while (lg > 6 && (1ull << lg) * 8 > free_b / 8) lg--;
    return (1ull << lg) * 64 >= n_kmers * 8 ? lg : 0;
}

// ---- neighbour words -------------------------------------------------------
// what may take three quarters of the free memory (the neighbour planes)
inline bool leaves_quarter(uint64_t bytes, uint64_t free_b) { return bytes <= free_b / 4 * 3; }

// One-substitution neighbours of one-word keys, 3 words per base: 8-B words
// (present | specific, 24 B per base) when that leaves a quarter of the free
// memory, else 4-B words (present only: a present neighbour is then probed),
// else none (0).  half (PA_NB_HALF=1) and the large layout force the 4-B form.
inline uint64_t nb_word_bytes(uint64_t n, uint64_t free_b, bool half, bool force_large) {
    const bool full = leaves_quarter(n * 24, free_b) && !half && !force_large;
    const uint64_t wb = full ? 8 : 4;
    return leaves_quarter(n * 3 * wb, free_b) ? wb : 0;
}

// The neighbour words in two pieces, when one allocation would have to give
// idle slabs back (the driver's reclaim of memory freed earlier runs ~60 GB/s:
// 1.9 s for C5's words after EXTSIM): the first piece as large as the pool's
// largest free range less 2 MiB (the second then from the free device memory),
// at most 7/8 of the words; usable when it is at least an eighth of them.
// force (PA_NB_SPLIT=1, tests): two halves.
struct NbSplit {
    uint64_t first;  // words of the first piece
    bool usable;
};
inline NbSplit nb_split(uint64_t words, uint64_t word_bytes, uint64_t pool_largest_free, bool force) {
    uint64_t w = force ? words / 2
                       : (pool_largest_free > (2ull << 20) ? (pool_largest_free - (2ull << 20)) / word_bytes : 0);
    w = std::min<uint64_t>(w, words - words / 8);
    return NbSplit{w, w >= words / 8};
}

}  // namespace plan
}  // namespace pa
