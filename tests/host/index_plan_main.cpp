// The index build's sizing plan (csrc/pa_index_plan.h) and the ownership list
// of an index's align-side view (release_align_view, dev_release:
// csrc/pa_internal.h) on the CPU.  The expected values are worked out by hand
// from the rules the comments of the plan state, at the sizes no GPU test
// reaches (C5: 8 G windows, 2.65 G distinct k-mers, 288 GB).  Built with
// -fsanitize=address,undefined by tests/test_index_plan_host.py: a leak, a
// double free or an overflowing shift ends the program with a report; exit
// status 0 means every check held.  No GPU and no HIP runtime: the allocator
// the helpers call is defined here, on malloc.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pa_index_plan.h"
#include "pa_internal.h"

namespace {
int g_failed = 0;
int g_frees = 0;  // calls of dev_free with a buffer

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)
#define CHECK_EQ(got, want)                                                                       \
    do {                                                                                          \
        const unsigned long long g_ = (unsigned long long)(got), w_ = (unsigned long long)(want); \
        if (g_ != w_) {                                                                           \
            fprintf(stderr, "%s:%d: %s = %llu, expected %llu\n", __FILE__, __LINE__, #got, g_, w_); \
            g_failed++;                                                                           \
        }                                                                                         \
    } while (0)

constexpr uint64_t KiB = 1ull << 10, MiB = 1ull << 20, GiB = 1ull << 30;
}  // namespace

namespace pa {
hipError_t dev_malloc_raw(void **p, size_t n) {
    *p = std::malloc(n);
    return hipSuccess;
}
hipError_t dev_free(void *p) {
    if (!p) return hipSuccess;
    g_frees++;
    std::free(p);
    return hipSuccess;
}
}  // namespace pa

extern "C" hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }

namespace plan = pa::plan;

static void table_on_windows() {
    const uint64_t ample = 1ull << 40;
    // 1,000 windows of one-word keys (16-B slots), ample memory: 4 per window + 64; compact: 2 per window + 64
    CHECK_EQ(plan::table_cap_windows(1000, 16, ample, false), 4 * 1000 + 64);
    CHECK_EQ(plan::table_cap_windows(1000, 16, ample, true), 2 * 1000 + 64);
    CHECK_EQ(plan::table_cap_windows(1000, 24, ample, false), 4 * 1000 + 64);  // (two-word keys: the same counts)
    // "table + build scratch fit": cap (slot + 20) + 4 windows + 1 GiB <= free.  10^6 windows, 16-B slots:
    //   4 per window: 4,000,064 * 36 + 4,000,000 + 2^30 = 1,221,744,128
    //   2 per window: 2,000,064 * 36 + 4,000,000 + 2^30 = 1,149,744,128
    CHECK(plan::table_fits(4000064, 16, 1000000, 1221744128ull));
    CHECK(!plan::table_fits(4000064, 16, 1000000, 1221744127ull));
    CHECK_EQ(plan::table_cap_windows(1000000, 16, 1221744128ull, false), 4000064);
    CHECK_EQ(plan::table_cap_windows(1000000, 16, 1221744127ull, false), 2000064);
    CHECK_EQ(plan::table_cap_windows(1000000, 16, 1149744128ull, false), 2000064);
    CHECK_EQ(plan::table_cap_windows(1000000, 16, 1149744127ull, false), 0);  // neither: the distinct estimate decides
    // "the table fits a third of the free memory": 10^8 windows, 4 per window = 400,000,064 slots of 16 B =
    // 6,400,001,024 B, a third of 19,200,003,072 (table + scratch need 15.9 GB only: this rule binds)
    CHECK_EQ(plan::table_cap_windows(100000000, 16, 19200003072ull, false), 400000064);
    CHECK_EQ(plan::table_cap_windows(100000000, 16, 19200003071ull, false), 200000064);
    // PA_CAP_MULT: that many per window, at least 2, whatever fits
    CHECK_EQ(plan::table_cap_windows(1000, 16, ample, false, 3), 3 * 1000 + 64);
    CHECK_EQ(plan::table_cap_windows(1000, 16, ample, true, 1), 2 * 1000 + 64);
    CHECK_EQ(plan::table_cap_windows(1000, 16, 0, false, 8), 8 * 1000 + 64);
    CHECK_EQ(plan::table_cap_windows(1000, 16, 0, false), 0);
    // whole 64-B lines: a multiple of 4 slots, never fewer than asked, an empty index keeps 64
    CHECK_EQ(plan::table_cap_lines(0), 64);
    CHECK_EQ(plan::table_cap_lines(4064), 4064);
    CHECK_EQ(plan::table_cap_lines(4065), 4068);
    for (uint64_t c = 1; c < 4000; c += 7) {
        const uint64_t r = plan::table_cap_lines(c);
        CHECK(r % 4 == 0 && r >= c && r - c < 4);
    }
}

static void table_on_distinct() {
    // C5: 8 * 10^9 windows, 2.65 * 10^9 distinct k-mers, 16-B slots, 288 GB.
    const uint64_t W = 8000000000ull, D = 2650000000ull, GB288 = 288000000000ull;
    // the first stage refuses both: 4 W slots of 16 B are 512 GB; 2 W slots need 36 B each = 576 GB
    CHECK_EQ(plan::table_cap_windows(W, 16, GB288, false), 0);
    CHECK_EQ(plan::table_cap_windows(W, 16, GB288, true), 0);
    // the second: c (16 + 20) + reserve <= free, reserve = 4 W + 2^30 = 33,073,741,824
    //   4    D + 64 = 10,600,000,064 -> 381,600,002,304 + reserve = 414,673,744,128
    //   2.5  D + 64 =  6,625,000,064 -> 238,500,002,304 + reserve = 271,573,744,128
    //   2    D + 64 =  5,300,000,064 -> 190,800,002,304 + reserve = 223,873,744,128
    //   1.43 D + 64 =  3,789,500,064 -> 136,422,002,304 + reserve = 169,495,744,128 (1.43 is no binary
    //                  fraction: the product may round one slot down)
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, GB288, false), 6625000064ull);  // C5 as it is built: load 0.4
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 414673744128ull, false), 10600000064ull);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 414673744127ull, false), 6625000064ull);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 271573744128ull, false), 6625000064ull);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 271573744127ull, false), 5300000064ull);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 223873744128ull, false), 5300000064ull);
    const uint64_t c143 = plan::table_cap_distinct(D, W, 16, 223873744127ull, false);
    CHECK(c143 == 3789500064ull || c143 == 3789500063ull);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 169495744128ull + 36, false), c143);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 169495744128ull - 37, false), 0);  // PA_ENOMEM's condition
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 0, false), 0);
    // forced (PA_CAP_HLL=1, PA_LAYOUT=large): never a multiplier above 1.5, however much memory
    const uint64_t frees[] = {1ull << 50, 414673744128ull, GB288, 223873744128ull, 170000000000ull};
    const double firsts[] = {0.0, 1.3, 1.5, 3.0, 8.0, 9.0};
    for (uint64_t f : frees)
        for (double m : firsts) {
            const uint64_t c = plan::table_cap_distinct(D, W, 16, f, true, m);
            CHECK(c != 0 && c <= D + D / 2 + 64);
            if (m != 1.3 && m != 1.5) CHECK_EQ(c, c143);
        }
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 169000000000ull, true), 0);
    // PA_CAP_DISTINCT: within [1.2, 8] it is tried first, then 2 and 1.43; outside, the list stands
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 1ull << 50, false, 3.0), 3 * D + 64);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, GB288, false, 3.0), 5300000064ull);  // 3 D needs 319 GB + reserve
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 1ull << 50, false, 8.0), 8 * D + 64);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 1ull << 50, false, 9.0), 4 * D + 64);
    CHECK_EQ(plan::table_cap_distinct(D, W, 16, 1ull << 50, false, 1.0), 4 * D + 64);
    // pass 1's list places: 4 B per base within an eighth of the free memory
    CHECK(plan::lpos_fits(1000, 32000) && !plan::lpos_fits(1000, 31999));
}

static void hyperloglog() {
    const uint32_t m = 1u << 16;
    const double alpha = 0.7213 / (1.0 + 1.079 / (double)m);
    std::vector<uint32_t> reg(m, 0);
    // no window seen: every register empty, the small-range form gives m ln(m / m) = 0
    CHECK_EQ(plan::hll_distinct(reg.data(), m), 64);
    // 1000 registers hit once (rank 1): the raw estimate (~0.73 m) is below 2.5 m and registers are
    // empty, so the estimate is m ln(m / empty) = 65536 ln(65536 / 64536) = 1007.7; + 3 % = 1037.9
    for (uint32_t i = 0; i < 1000; i++) reg[i * 64] = 1;
    CHECK_EQ(plan::hll_distinct(reg.data(), m), 1037 + 64);
    CHECK_EQ(plan::hll_distinct(reg.data(), m), (uint64_t)((double)m * std::log((double)m / 64536.0) * 1.03) + 64);
    // every register at rank r: sum 2^-reg = m 2^-r, no register empty -> alpha m 2^r (+ 3 %), also
    // where that is below 2.5 m (the correction needs an empty register)
    for (int r : {1, 10, 20}) {
        for (auto &v : reg) v = (uint32_t)r;
        const uint64_t got = plan::hll_distinct(reg.data(), m);
        const uint64_t want = (uint64_t)(alpha * (double)m * std::ldexp(1.0, r) * 1.03) + 64;
        CHECK(got + 1 >= want && got <= want + 1);
        // alpha = 0.72129 at m = 2^16: within a slot of 0.72129 * 1.03 * 2^(16 + r)
        CHECK(std::fabs((double)(got - 64) / std::ldexp(1.0, 16 + r) - 0.742927) < 1e-5);
    }
    // a small register file (the function takes any size): 16 registers, 8 of them hit -> 16 ln 2 = 11.09, + 3 % = 11.4
    std::vector<uint32_t> small(16, 0);
    for (int i = 0; i < 8; i++) small[2 * i] = 3;
    CHECK_EQ(plan::hll_distinct(small.data(), 16), 11 + 64);
}

static void blooms() {
    const uint64_t ample = 1ull << 45;
    // the neighbour-bit build's filter: the smallest lg >= 6 with 4 * 2^lg >= n_kmers, ...
    CHECK_EQ(plan::nb_bloom_lg(0, ample), 0);
    CHECK_EQ(plan::nb_bloom_lg(1, ample), 6);
    CHECK_EQ(plan::nb_bloom_lg(256, ample), 6);
    CHECK_EQ(plan::nb_bloom_lg(257, ample), 7);
    CHECK_EQ(plan::nb_bloom_lg(1ull << 20, ample), 18);
    CHECK_EQ(plan::nb_bloom_lg((1ull << 20) + 1, ample), 19);
    // ... shrunk to a quarter of the free memory (2^lg words of 8 B), accepted at 8 bits per key or more:
    // 2^20 keys need lg >= 17 (1 MiB)
    CHECK_EQ(plan::nb_bloom_lg(1ull << 20, 8 * MiB), 18);
    CHECK_EQ(plan::nb_bloom_lg(1ull << 20, 8 * MiB - 1), 17);
    CHECK_EQ(plan::nb_bloom_lg(1ull << 20, 4 * MiB), 17);
    CHECK_EQ(plan::nb_bloom_lg(1ull << 20, 4 * MiB - 1), 0);
    CHECK_EQ(plan::nb_bloom_lg(1ull << 20, 0), 0);
    CHECK_EQ(plan::nb_bloom_lg(512, 0), 6);  // (64 words hold 8 bits each of 512 keys; lg never goes below 6)
    CHECK_EQ(plan::nb_bloom_lg(513, 0), 0);
    // lg <= 33: 2^35 keys reach it at 16 bits per key, 2^36 at 8 (64 GiB: a quarter of 256 GiB), one more is refused
    CHECK_EQ(plan::nb_bloom_lg(1ull << 35, ample), 33);
    CHECK_EQ(plan::nb_bloom_lg((1ull << 35) + 1, ample), 33);
    CHECK_EQ(plan::nb_bloom_lg(1ull << 36, 256 * GiB), 33);
    CHECK_EQ(plan::nb_bloom_lg(1ull << 36, 256 * GiB - 1), 0);
    CHECK_EQ(plan::nb_bloom_lg((1ull << 36) + 1, ample), 0);

    // the align-side filter, cache-sized: 16 bits per key (64 * 2^lg >= 16 n) within 128 MiB (lg <= 24), down to 8
    plan::BloomSwitches def;
    CHECK_EQ(plan::align_bloom_lg_cache(0, def), 0);
    CHECK(!plan::align_bloom_hbm_wanted(0, def));
    CHECK_EQ(plan::align_bloom_lg_cache(1, def), 6);
    CHECK_EQ(plan::align_bloom_lg_cache(1ull << 20, def), 18);
    CHECK_EQ(plan::align_bloom_lg_cache((1ull << 20) + 1, def), 19);
    CHECK_EQ(plan::align_bloom_lg_cache(1ull << 26, def), 24);
    CHECK_EQ(plan::align_bloom_lg_cache(1ull << 27, def), 24);  // 8 bits per key
    CHECK_EQ(plan::align_bloom_lg_cache((1ull << 27) + 1, def), 0);
    CHECK(plan::align_bloom_hbm_wanted((1ull << 27) + 1, def));
    // ... then in HBM: 16 bits per key (lg 26 = 512 MiB) in an eighth of the free memory, down to 8 (lg 25)
    CHECK_EQ(plan::align_bloom_lg_hbm((1ull << 27) + 1, ample), 26);
    CHECK_EQ(plan::align_bloom_lg_hbm((1ull << 27) + 1, 4 * GiB), 26);
    CHECK_EQ(plan::align_bloom_lg_hbm((1ull << 27) + 1, 4 * GiB - 1), 25);
    CHECK_EQ(plan::align_bloom_lg_hbm((1ull << 27) + 1, 2 * GiB), 25);
    CHECK_EQ(plan::align_bloom_lg_hbm((1ull << 27) + 1, 2 * GiB - 1), 0);
    CHECK_EQ(plan::align_bloom_lg_hbm(1ull << 36, ample), 33);
    CHECK_EQ(plan::align_bloom_lg_hbm((1ull << 36) + 1, ample), 0);
    // the switches
    plan::BloomSwitches mb64 = def, mb0 = def, no_hbm = def, large = def, large_mb = def;
    mb64.mb_set = true, mb64.mb = 64;
    CHECK_EQ(plan::align_bloom_lg_cache(1ull << 26, mb64), 23);  // 64 MiB: 8 bits per key
    CHECK_EQ(plan::align_bloom_lg_cache((1ull << 26) + 1, mb64), 0);
    CHECK(!plan::align_bloom_hbm_wanted((1ull << 26) + 1, mb64));  // a given size means that size or none
    mb0.mb_set = true, mb0.mb = 0;
    CHECK_EQ(plan::align_bloom_lg_cache(1000, mb0), 0);
    CHECK(!plan::align_bloom_hbm_wanted(1000, mb0));
    no_hbm.hbm_off = true;
    CHECK_EQ(plan::align_bloom_lg_cache(1000, no_hbm), 6 + 2);  // 16,000 bits: 256 words
    CHECK(!plan::align_bloom_hbm_wanted(1ull << 30, no_hbm));
    large.force_large = true;
    CHECK_EQ(plan::align_bloom_lg_cache(1000, large), 0);
    CHECK(plan::align_bloom_hbm_wanted(1000, large));
    large_mb.force_large = true, large_mb.mb_set = true, large_mb.mb = 64;
    CHECK_EQ(plan::align_bloom_lg_cache(1000, large_mb), 0);
    CHECK(plan::align_bloom_hbm_wanted(1000, large_mb));
    large_mb.hbm_off = true;
    CHECK(!plan::align_bloom_hbm_wanted(1000, large_mb));
}

static void neighbour_words() {
    // 3 words per base: 8-B words when 24 n leaves a quarter of the free memory, else 4-B words when 12 n does, else none
    CHECK_EQ(plan::nb_word_bytes(1000, 1ull << 40, false, false), 8);
    CHECK_EQ(plan::nb_word_bytes(1000, 1ull << 40, true, false), 4);   // PA_NB_HALF=1
    CHECK_EQ(plan::nb_word_bytes(1000, 1ull << 40, false, true), 4);   // the large layout
    CHECK_EQ(plan::nb_word_bytes(1000, 32000, false, false), 8);       // 24,000 = 3/4 of 32,000
    CHECK_EQ(plan::nb_word_bytes(1000, 31999, false, false), 4);
    CHECK_EQ(plan::nb_word_bytes(1000, 16000, false, false), 4);       // 12,000 = 3/4 of 16,000
    CHECK_EQ(plan::nb_word_bytes(1000, 16000, true, false), 4);
    CHECK_EQ(plan::nb_word_bytes(1000, 15999, false, false), 0);
    CHECK_EQ(plan::nb_word_bytes(1000, 15999, true, true), 0);
    // C5's 8 * 10^9 bases: 192 GB of full words never fit 3/4 of 288 GB less the 87 GB table; half words (96 GB) do
    CHECK_EQ(plan::nb_word_bytes(8000000000ull, 200000000000ull, false, false), 4);
    CHECK(plan::leaves_quarter(96000000000ull, 128000000000ull) && !plan::leaves_quarter(96000000000ull, 127999999999ull));
    // two pieces: the first as large as the pool's largest free range less 2 MiB, at most 7/8 of the
    // words, usable from 1/8 of them
    const uint64_t words = 8000;
    plan::NbSplit s = plan::nb_split(words, 8, 1ull << 40, false);
    CHECK_EQ(s.first, 7000);
    CHECK(s.usable);
    s = plan::nb_split(words, 8, 2 * MiB + 7000 * 8, false);
    CHECK_EQ(s.first, 7000);
    s = plan::nb_split(words, 8, 2 * MiB + 7000 * 8 - 1, false);
    CHECK_EQ(s.first, 6999);
    s = plan::nb_split(words, 8, 2 * MiB + 1000 * 8, false);
    CHECK_EQ(s.first, 1000);
    CHECK(s.usable);
    s = plan::nb_split(words, 8, 2 * MiB + 1000 * 8 - 1, false);
    CHECK_EQ(s.first, 999);
    CHECK(!s.usable);
    s = plan::nb_split(words, 4, 2 * MiB + 1000 * 4, false);
    CHECK_EQ(s.first, 1000);
    CHECK(s.usable);
    for (uint64_t lf : {(uint64_t)0, 64 * KiB, 2 * MiB}) {
        s = plan::nb_split(words, 8, lf, false);
        CHECK_EQ(s.first, 0);
        CHECK(!s.usable);
    }
    for (uint64_t lf : {(uint64_t)0, 1024 * GiB}) {  // PA_NB_SPLIT=1: two halves, whatever the pool holds
        s = plan::nb_split(words, 8, lf, true);
        CHECK_EQ(s.first, 4000);
        CHECK(s.usable);
    }
}

template <typename T>
static void fill(T *&p) {
    CHECK(pa::dev_malloc(&p, 64) == hipSuccess && p != nullptr);
}

static void ownership() {
    {  // dev_release: freed and forgotten
        uint32_t *p = nullptr;
        fill(p);
        g_frees = 0;
        pa::dev_release(p);
        CHECK(p == nullptr && g_frees == 1);
        pa::dev_release(p);
        CHECK(g_frees == 1);
    }
    pa_index idx;
    // every buffer of the align-side view held, every state field away from its initial value
    fill(idx.tile_cls), fill(idx.tile_pk), fill(idx.tile_lw), fill(idx.tile_gblk);
    fill(idx.tile_nb), fill(idx.tile_nb1), fill(idx.tile_rcnb);
    fill(idx.bloom), fill(idx.mm_bits), fill(idx.tile_rcp);
    fill(idx.tile_big), fill(idx.tile_nbbig), fill(idx.tile_nbm);
    idx.tile_n = 12345, idx.nb_split = 17, idx.nb_spec = 1, idx.nb_pending = 1, idx.rcnb_pending = 1;
    idx.rcnb_checks = 3, idx.bloom_lg = 20, idx.mm_lg = 25;
    idx.tile_big_mg = 2, idx.tile_nbbig_mg = 3, idx.tile_nbm_mg = 4;
    // what is not the align-side view stays
    fill(idx.table);
    idx.n_kmers = 99, idx.cap = 128, idx.reads_seen = 7;
    g_frees = 0;
    pa::release_align_view(&idx);
    CHECK_EQ(g_frees, 13);
    CHECK(!idx.tile_cls && !idx.tile_pk && !idx.tile_lw && !idx.tile_gblk);
    CHECK(!idx.tile_nb && !idx.tile_nb1 && !idx.tile_rcnb);
    CHECK(!idx.bloom && !idx.mm_bits && !idx.tile_rcp);
    CHECK(!idx.tile_big && !idx.tile_nbbig && !idx.tile_nbm);
    CHECK_EQ(idx.tile_n, 0);
    CHECK_EQ(idx.nb_split, ~0ull);
    CHECK(idx.nb_spec == 0 && idx.nb_pending == 0 && idx.rcnb_pending == 0 && idx.rcnb_checks == 0);
    CHECK(idx.bloom_lg == 0 && idx.mm_lg == 0);
    CHECK(idx.tile_big_mg == -1 && idx.tile_nbbig_mg == -1 && idx.tile_nbm_mg == -1);
    CHECK(idx.table != nullptr && idx.n_kmers == 99 && idx.cap == 128 && idx.reads_seen == 7);
    pa::release_align_view(&idx);  // again: nothing to free
    CHECK_EQ(g_frees, 13);
    pa::dev_release(idx.table);
    CHECK(idx.table == nullptr && g_frees == 14);
}

int main() {
    table_on_windows();
    table_on_distinct();
    hyperloglog();
    blooms();
    neighbour_words();
    ownership();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    printf("index plan ok\n");
    return 0;
}
