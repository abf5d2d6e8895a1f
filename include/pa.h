/*
 * pa.h -- C ABI of libpa.so, the MI355X (gfx950) pseudo-alignment engine.
 *
 * The reference (nyenyu12/BioInformatics-project-for-Shotgun-Metagenomics-
 * Pseudo-alignment-shotgun-, pure Python) has no FFI; its boundary for this
 * path is the Python API of src/kmer.py plus the dumpalign CLI.  Each entry
 * point below replaces one piece of that API (file:line in the reference):
 *
 *   pa_index_build           KmerReference.__init__ / _build_kmer_mapping   src/kmer.py:113-150
 *   pa_index_build_ex        the same, the align-side view deferred        src/kmer.py:113-133
 *   pa_index_reduce          KmerReference._filter_similar_genomes (pruning)  src/kmer.py:232-263
 *   pa_index_prepare         (the deferred view, before the first align)
 *   pa_index_prepare_ex      the same, sized for the reads the caller expects
 *   pa_params_effective      the filters a batch's align applies (Read.mean_quality /
 *                            kmer_quality thresholds no read can fail) src/kmer.py:394-408
 *   pa_index_lookup          KmerReference.get_kmer_references / __getitem__ src/kmer.py:284-298
 *   pa_index_class_genomes   (genome set of a k-mer, i.e. the keys of kmers[kmer]) src/kmer.py:130
 *   pa_index_positions       KmerReference.get_kmer_references (positions) and
 *                            get_kmer_and_reverse_references              src/kmer.py:292-298, 331-351
 *   pa_index_dumpref         KmerReference.get_summary ("Kmers" + Summary counts)
 *                            streamed as JSON text (dumpref)                src/kmer.py:300-329
 *   pa_index_extsim_stats    KmerReference._compute_genome_stats + the pairwise
 *                            intersections of _apply_greedy_filter          src/kmer.py:152-230
 *   pa_align                 PseudoAlignment.align_reads_from_container ->
 *                            Read.pseudo_align (counters only)              src/kmer.py:482-620
 *   pa_align_detail          the same, with per-read mapping type and
 *                            genomes_mapped_to (PseudoAlignment.reads)      src/kmer.py:542, 551-561
 *   pa_align_reads           the same per-read results for a whole batch at
 *                            about the counter pass's cost: the lane kernels
 *                            write the reads they settle, the exact kernel the
 *                            rest (PseudoAlignment.reads, --assignments)    src/kmer.py:542, 551-561
 *   pa_result_fetch          PseudoAlignment.get_summary inputs             src/kmer.py:622-657
 *   pa_align_pairs           paired-end reads: a pair classified as one fragment by the union of both
 *                            mates' k-mers (--reads2); no reference counterpart: the definition is
 *                            DESIGN.md section 15 (the decision is src/kmer.py:444-480 unchanged)
 *   pa_coverage_* /          the course project's EXTCOVERAGE extension (--coverage, --genomes,
 *   pa_align_placements      --min-coverage, --full-coverage), which the reference leaves out: it
 *                            has no coverage code, so the definition is DESIGN.md section 10; the
 *                            occurrence sets it places reads with are kmers[w][g], src/kmer.py:140-150
 *   pa_pileup_*              per-base counts and SNV calls from the uniquely mapped reads (--variants);
 *                            no reference counterpart: the definition is DESIGN.md section 13
 *   pa_abundance_* /         what is in the sample and in what proportions (--abundance): the reads'
 *   pa_align_candidates      compatibility classes and an EM over them; no reference counterpart: the
 *                            definition is DESIGN.md section 14 (T_r(g) is generate_genome_counts(
 *                            map_count=False), src/kmer.py:431-442)
 *   pa_lineage_*             every read's node in a taxonomy tree (the lowest common ancestor of its
 *                            compatibility set) and the reads per node and clade (--lineages); no
 *                            reference counterpart: the definition is DESIGN.md section 17
 *   pa_containment_*         the distinct reference k-mers the reads hold, per genome and per node of
 *                            a lineage tree (--containment); no reference counterpart: the definition
 *                            is DESIGN.md section 21 (the windows are extract_kmer_references',
 *                            src/kmer.py:410-429)
 *   pa_align_batch           one-shot host-buffer form of pa_align
 *   pa_align_fastq_file      FASTAQFile + align_reads_from_container as one
 *                            device-parsed stream                          src/data_file.py:134-158,
 *                                                                          src/kmer.py:600-620
 *   pa_align_fastq_range     the same over a byte range of the file, one per device:
 *   pa_idsets_disjoint       the dumpalign job read-sharded over N GPUs     src/main.py:289-310
 *   pa_fastq_prefetch_start  the same with the file moved to the device in the
 *   pa_align_fastq_prefetched  background (overlaps the index build)       src/main.py:286-310
 *   pa_extract_fastq_file    the same stream with the selected records written back out as FASTQ
 *   pa_reads_select          (--extract: host depletion, the reads of one genome, the unmapped reads);
 *                            no reference counterpart: the definition is DESIGN.md section 20
 *   pa_reads_trim            quality ends and a 3' adapter cut off every read on the device
 *   pa_*_fastq_*_ex          (--trim-*), for a batch and per window of the three streams above;
 *                            no reference counterpart: the definition is DESIGN.md section 22
 *   pa_counters_reduce       the multi-GPU sum/min of PseudoAlignment counters
 *                            (read shards of one job); the
 *                            reference is single-process, so this has no
 *                            reference counterpart: it makes N per-rank
 *                            get_summary inputs equal to the one-process ones
 *                            src/kmer.py:622-657
 *   pa_parse_file/_text      FASTAFile / FASTAQFile -> FASTARecordContainer /
 *                            FASTAQRecordContainer.parse_records (host
 *                            threads, canonical subset of the grammar)     src/data_file.py:117-158,
 *                                                                          src/records.py:141-302
 *
 * Conventions
 *   - Every function returns PA_OK (0) or an error code; pa_last_error()
 *     gives a thread-local message.  The Python layer maps PA_EINVAL to
 *     ValueError and PA_ETYPE to TypeError, like src/kmer.py:501-510.
 *   - Buffers named seq/qual/genomes/read_off/... are HOST pointers; the
 *     library copies them.  Objects (pa_index, pa_reads, pa_result) own DEVICE
 *     memory on the device they were created on.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream).  All work is
 *     stream-ordered; functions that return host data synchronize that stream.
 *   - Calls on one pa_index are not thread-safe with respect to each other.
 *   - Genome text must be uppercase ACGTN (the FASTA grammar,
 *     src/records.py:225-233); reads may contain any byte, but only ACGT
 *     windows can match (the FASTQ grammar restricts reads to ACGT,
 *     src/records.py:258-265).
 *   - Mapping types use the reference's enum values (src/kmer.py:41-47):
 *     1 UNMAPPED, 2 UNIQUELY_MAPPED, 3 AMBIGUOUSLY_MAPPED; 0 marks a read
 *     dropped by --min-read-quality (src/kmer.py:587-589: not in `reads`).
 */
#ifndef PA_H
#define PA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t pa_status;
#define PA_OK 0
#define PA_EINVAL 1        /* bad argument value (ValueError) */
#define PA_ETYPE 2         /* bad argument kind (TypeError) */
#define PA_ENOMEM 3        /* host or device allocation failed */
#define PA_EDEVICE 4       /* HIP runtime error */
#define PA_EUNSUPPORTED 5  /* e.g. k > PA_MAX_K */
#define PA_EINTERNAL 6     /* invariant violated (reported, never silent) */
#define PA_ENOTCANON 7     /* ingest: text outside the canonical FASTA/FASTQ subset (use the exact grammar) */
#define PA_EIO 8           /* ingest: file could not be opened / read */

#define PA_MAX_K 255       /* k-mers up to 255 bases: keys of up to 8 x 64-bit words */

#define PA_DROPPED 0
#define PA_UNMAPPED 1
#define PA_UNIQUELY_MAPPED 2
#define PA_AMBIGUOUSLY_MAPPED 3

/* pa_params.flags: which optional EXTQUALITY arguments are set (not None) */
#define PA_HAS_MIN_READ_QUALITY 1u
#define PA_HAS_MIN_KMER_QUALITY 2u
#define PA_HAS_MAX_GENOMES 4u

#define PA_NO_FIRST_KEY INT64_MAX  /* first_key of a genome never counted; all keys are < 2^63 */
/* first_key = (global read index << 20) | position in that read's
 * genomes_mapped_to list (<= G: a p-demoted list holds G* twice), so an index
 * holds at most PA_MAX_GENOMES genomes (pa_index_build: PA_EUNSUPPORTED above)
 * and read indices stay below 2^43. */
#define PA_MAX_GENOMES ((1u << 20) - 1)

typedef struct pa_index pa_index;
typedef struct pa_reads pa_reads;
typedef struct pa_result pa_result;

/* Arguments of Read.pseudo_align / align_reads_from_container (src/kmer.py:482-489, 600-606). */
typedef struct {
    int64_t m;                 /* unique threshold; < 0 -> PA_EINVAL (src/kmer.py:509-510) */
    int64_t p;                 /* ambiguity threshold; < 0 skips validation (src/kmer.py:469) */
    int64_t min_read_quality;  /* raw-ASCII mean, strict < (src/kmer.py:399, 587) */
    int64_t min_kmer_quality;  /* raw-ASCII window mean, strict < (src/kmer.py:408, 420) */
    int64_t max_genomes;       /* genomes per k-mer, strict > (src/kmer.py:425) */
    uint32_t flags;            /* PA_HAS_* */
    uint32_t reserved;
} pa_params;

/* "Statistics" of get_summary (src/kmer.py:627-637). */
typedef struct {
    uint64_t unique_mapped_reads;
    uint64_t ambiguous_mapped_reads;
    uint64_t unmapped_reads;
    uint64_t filtered_quality_reads;
    uint64_t filtered_quality_kmers;   /* windows, repeats included (quirk 4) */
    uint64_t filtered_hr_kmers;        /* windows, repeats included (quirk 4) */
} pa_stats;

typedef struct {
    uint32_t k;
    uint32_t n_genomes;
    uint32_t key_words;            /* 64-bit words per packed k-mer key */
    uint32_t slot_bytes;
    uint64_t n_kmers;              /* distinct k-mers (len(KmerReference.kmers)) */
    uint64_t n_multi_classes;      /* distinct genome sets with >= 2 genomes */
    uint64_t class_genome_entries;
    uint64_t table_slots;
    uint64_t table_bytes;
    uint64_t total_windows;        /* genome windows scanned by the build */
    uint64_t device_bytes;         /* all device memory held by the index */
} pa_index_info;

const char *pa_last_error(void);
const char *pa_version(void);
pa_status pa_device_count(int32_t *n);

/* ---- index (KmerReference) ---------------------------------------------- */

/* genomes: concatenated ASCII; genome_off: n_genomes+1 offsets (CSR). */
pa_status pa_index_build(int32_t device, const char *genomes, const uint64_t *genome_off, uint32_t n_genomes,
                         int64_t k, void *stream, pa_index **out);
/* The same with build flags.  PA_BUILD_DEFER_TILES: build the k-mer table and
 * the genome sets only; the align-side view (genome tiling, neighbour bits,
 * Bloom filter -- DESIGN.md section 3) is made by pa_index_prepare or by the
 * first pa_align / pa_align_detail call.  For an index that may only feed
 * pa_index_extsim_stats (KmerReference(..., filter_similar=True) builds, then
 * filters: src/kmer.py:113-133, 252-263) before it is rebuilt from the kept
 * genomes.  pa_index_build = pa_index_build_ex(..., 0, ...). */
#define PA_BUILD_DEFER_TILES 1u
/* PA_BUILD_COMPACT: the k-mer table at 2 slots per genome window (default 4;
 * for k <= 31: longer keys, and a table sized on the distinct k-mers, too
 * large for 2 per window, are not changed) -- builds faster, aligns
 * slightly slower (MI355X, round 6: C4 build 0.453 -> 0.395 s, its align pass
 * +4 %; C2 0.057 -> 0.048 s, +3 %).  For a job of fewer than
 * PA_COMPACT_READS_PER_BASE reads per genome base (the measured break-even,
 * 3-5): the CLI's dumpalign job, bench.py's job index.  Results never depend
 * on it.  Kept by pa_index_reduce when given again in its flags. */
#define PA_BUILD_COMPACT 2u
#define PA_COMPACT_READS_PER_BASE 3
/* PA_BUILD_BOTH_STRANDS: a both-strand (reverse-complement aware) index.  The
 * genome set of a k-mer w becomes S(w) | S(rc(w)), S the forward index's set --
 * the merge of get_kmer_and_reverse_references (src/kmer.py:331-351), which the
 * reference's parsed-and-unused --reverse-complement flag (src/main.py:76)
 * never reached the align path with.  The device holds genome g as the region
 * T(g) = g + "N" + reverse_complement(g) (N's complement is N, an empty genome
 * stays empty; windows with an N are not indexed, src/kmer.py:145), made on
 * the device from the forward text, and every result -- pa_index_lookup,
 * pa_index_class_genomes, pa_index_extsim_stats, every pa_align* entry, their
 * counters, first keys and filter counters -- is bit for bit that of a forward
 * index of the genomes T(g_0) .. T(g_G-1).  In pa_index_info, n_kmers counts the
 * distinct k-mers over both strands, total_windows is twice the forward value,
 * and the other fields describe what is held: about twice a forward index's
 * table, tiles and device_bytes (a genome may hold < 2^31 bases for the tiling).
 * What speaks in genome coordinates stays forward: pa_index_positions (with or
 * without PA_POS_REVERSE) and pa_reads_synthesize[_mix] give exactly what a
 * forward index of the same genomes gives; pa_index_dumpref, the dump of the
 * forward k-mer database, is PA_EUNSUPPORTED (dump from a forward index).
 * Strandness is fixed at the build: pa_index_reduce keeps it, and does not
 * take this bit in its flags (PA_EINVAL). */
#define PA_BUILD_BOTH_STRANDS 4u
pa_status pa_index_build_ex(int32_t device, const char *genomes, const uint64_t *genome_off, uint32_t n_genomes,
                            int64_t k, uint32_t flags, void *stream, pa_index **out);
/* Rebuild an index over some of its own genomes, in place: their 2-bit codes
 * are gathered on the device (nothing is concatenated or uploaded again), the
 * rest of the index is released and built anew -- the EXTSIM rebuild of
 * KmerReference(filter_similar=True), where the reference deletes the dropped
 * genomes from its dict (src/kmer.py:232-263).  keep: n_keep ascending genome
 * numbers (< n_genomes); flags as pa_index_build_ex.  On failure the index
 * holds nothing and may only be freed. */
pa_status pa_index_reduce(pa_index *idx, const uint32_t *keep, uint32_t n_keep, uint32_t flags, void *stream);
/* Make a deferred build's align-side view now, with the neighbour bits a
 * pa_index_prepare_ex or a FASTQ prefetch left pending (no-op otherwise);
 * returns when it is done. */
pa_status pa_index_prepare(pa_index *idx, void *stream);
/* The same for a job of about expected_reads reads (PA_READS_UNKNOWN: as
 * pa_index_prepare).  The one-substitution neighbour bits (DESIGN.md section
 * 3) cost time per genome base and save time per read: below the break-even
 * (PA_NB_READS_PER_KBASE[_2W/_3W] reads per 1000 genome bases) they are left out, and made by
 * the align that brings the reads aligned with this index past that point --
 * or by a later call of this function whose expected_reads (the reads still to
 * come) passes it.  Results never depend on them.  Returns when done. */
#define PA_READS_UNKNOWN UINT64_MAX
/* the measured break-even (bench.py neighbour_bits_breakeven, MI355X, round 6,
 * reverse-complement bits made lazily), reads per 1000 genome bases: keys of
 * one word (k <= 31; C2 1.45, C4 2.05, C5 2.80 reads per base), two words
 * (31 < k <= 63: c2k63 10.3) and three (63 < k <= 95: c2k75 18.5) */
#define PA_NB_READS_PER_KBASE 2500
#define PA_NB_READS_PER_KBASE_2W 10000
#define PA_NB_READS_PER_KBASE_3W 18000
pa_status pa_index_prepare_ex(pa_index *idx, uint64_t expected_reads, void *stream);
void pa_index_free(pa_index *idx);
pa_status pa_index_get_info(const pa_index *idx, pa_index_info *out);
/* *both = 1 for an index built with PA_BUILD_BOTH_STRANDS, else 0. */
pa_status pa_index_strands(const pa_index *idx, uint32_t *both);
/* n k-mers of length kmer_len packed back to back; cls_out[i] = class id or -1
 * if absent; size_out[i] = number of genomes containing it (0 if absent). */
pa_status pa_index_lookup(const pa_index *idx, const char *kmers, uint64_t n, uint32_t kmer_len,
                          int64_t *cls_out, uint32_t *size_out, void *stream);
/* genome indices (ascending = FASTA order) of class `cls`; *n = class size. */
pa_status pa_index_class_genomes(const pa_index *idx, int64_t cls, uint32_t *genomes, uint32_t cap, uint32_t *n,
                                 void *stream);
/* Positions of n k-mers (kmer_len bases each, back to back) in the genomes:
 * every (query, genome, genome-local position) whose window holds the k-mer --
 * kmers[kmer] = {genome: positions} of the reference (src/kmer.py:140-150,
 * 292-298).  With PA_POS_REVERSE also every window holding its reverse
 * complement, unless that is the k-mer itself (get_kmer_and_reverse_references,
 * src/kmer.py:331-351); such hits carry PA_POS_RC_BIT in `query`.  A k-mer of
 * another length than the index's k, or with anything but A/C/G/T, has none.
 * Hits are sorted by (query, strand, genome, position); *n_hits = all of them,
 * of which the first min(cap, *n_hits) are written (hits may be NULL to count).
 * Genomes are numbered as built (after EXTSIM: the kept genomes). */
#define PA_POS_REVERSE 1u
#define PA_POS_RC_BIT 0x80000000u
typedef struct {
    uint32_t query;     /* query index | PA_POS_RC_BIT for a reverse-complement hit */
    uint32_t genome;
    uint64_t position;  /* window start within the genome */
} pa_kmer_hit;
pa_status pa_index_positions(const pa_index *idx, const char *kmers, uint64_t n, uint32_t kmer_len, uint32_t flags,
                             pa_kmer_hit *hits, uint64_t cap, uint64_t *n_hits, void *stream);
/* EXTSIM inputs at identifier-group granularity (group_of[n_genomes]):
 * total[a] = distinct k-mers touching group a, uniq[a] = k-mers contained in
 * exactly one genome which belongs to a, inter[a*n_groups+b] = k-mers touching
 * both groups a != b. */
pa_status pa_index_extsim_stats(const pa_index *idx, const uint32_t *group_of, uint32_t n_groups, uint64_t *total,
                                uint64_t *uniq, uint64_t *inter, void *stream);

/* ---- reads ------------------------------------------------------------------ */

pa_status pa_reads_upload(int32_t device, const uint8_t *seq, const uint8_t *qual, const uint64_t *read_off,
                          uint64_t n_reads, void *stream, pa_reads **out);
/* Synthetic fixed-length forward-strand reads sampled on the device from the
 * index's genomes (read i = global read first_read + i; deterministic in seed). */
pa_status pa_reads_synthesize(const pa_index *idx, uint64_t n_reads, uint32_t read_len, uint64_t first_read,
                              uint64_t seed, double sub_rate, void *stream, pa_reads **out);
/* The same with a share of reverse-complemented reads (rc_rate: the reference
 * looks up forward k-mers only, so these mostly go unmapped) and of reads of
 * uniform random bases (foreign_rate: an organism absent from the index); the
 * rest forward.  rc_rate + foreign_rate <= 1.  (The robustness workload.) */
pa_status pa_reads_synthesize_mix(const pa_index *idx, uint64_t n_reads, uint32_t read_len, uint64_t first_read,
                                  uint64_t seed, double sub_rate, double rc_rate, double foreign_rate, void *stream,
                                  pa_reads **out);
pa_status pa_reads_info(const pa_reads *reads, uint64_t *n_reads, uint64_t *n_bases, uint32_t *max_len);
/* The filter arguments a pa_align of this batch applies (out, may alias in):
 * a --min-read-quality / --min-kmer-quality at or below the batch's smallest
 * quality byte can filter nothing (strict <, src/kmer.py:420, 587; quirk 5)
 * and is dropped from the pass -- its flag cleared, the counters unchanged.
 * q_min (nullable): that byte (255: no quality bytes). */
pa_status pa_params_effective(const pa_reads *reads, const pa_params *in, pa_params *out, int32_t *q_min,
                              void *stream);
/* copy reads [first, first+count) back to the host (seq/qual: n_bases of that range) */
pa_status pa_reads_download(const pa_reads *reads, uint64_t first, uint64_t count, uint8_t *seq, uint8_t *qual,
                            uint64_t *read_off, void *stream);
void pa_reads_free(pa_reads *reads);

/* Read trimming: quality ends, then a 3' adapter; integers only.
 * A read S, Q of length L becomes S[start:end], Q[start:end] (same index, nothing reordered
 * or removed; a read trimmed to nothing is an ordinary read of length 0):
 *   quality (BWA's running sum, both scans over the ORIGINAL read)
 *     cut = L; s = best = 0                          with PA_TRIM_QUALITY3
 *     for i = L-1 down to 0: s += quality3 - Q[i]; if s < 0: break; if s > best: best = s, cut = i
 *     start = 0; s = best = 0                        with PA_TRIM_QUALITY5
 *     for i = 0 .. L-1:      s += quality5 - Q[i]; if s < 0: break; if s > best: best = s, start = i + 1
 *     start >= cut: the read is empty, start = end = 0
 *   adapter A (3', Hamming distance, no indels) over R = S[start:cut] of length L'
 *     p = 0 .. L'-1 is a hit when ov = min(L' - p, |A|) >= min_overlap and
 *     1000 * mm <= max_error_permille * ov, mm = #{j < ov: R[p+j] != A[j]} (a read byte other
 *     than ACGT always mismatches); the smallest hit p wins: end = start + p; no hit: end = cut
 * Quality cutoffs are raw quality bytes, as pa_params.min_read_quality. */
#define PA_TRIM_MAX_ADAPTER 64
#define PA_TRIM_QUALITY3 1u
#define PA_TRIM_QUALITY5 2u
#define PA_TRIM_ADAPTER 4u
typedef struct {
    uint32_t flags, quality3, quality5, adapter_len, min_overlap, max_error_permille;
    char adapter[PA_TRIM_MAX_ADAPTER];
} pa_trim_spec;
/* Sums over reads (they do not depend on batching): reads_trimmed: length changed;
 * bases_quality: L - (cut - start), L for a read emptied by quality; bases_adapter: cut - end;
 * reads_empty: reads of length 0 afterwards. */
typedef struct {
    uint64_t reads, bases_in, bases_out, reads_trimmed, reads_quality, bases_quality, reads_adapter,
        bases_adapter, reads_empty;
} pa_trim_stats;
/* out: a new batch on in's device.  start / end: host [n] each, nullable, in the
 * original read's coordinates.  stats: nullable, ACCUMULATES.  flags == 0: an
 * identical copy.  PA_EINVAL: a NULL argument; an unknown flag; with
 * PA_TRIM_ADAPTER an adapter byte outside ACGT, adapter_len 0 or >
 * PA_TRIM_MAX_ADAPTER; min_overlap 0; max_error_permille > 500; a quality
 * cutoff > 255 (the last three whatever the flags). */
pa_status pa_reads_trim(const pa_reads *in, const pa_trim_spec *spec, pa_reads **out, uint32_t *start,
                        uint32_t *end, pa_trim_stats *stats, void *stream);

/* ---- results (PseudoAlignment counters) ------------------------------------- */

pa_status pa_result_create(const pa_index *idx, pa_result **out);
pa_status pa_result_reset(pa_result *res, void *stream);
/* any output pointer may be NULL; per-genome arrays hold n_genomes entries */
pa_status pa_result_fetch(const pa_result *res, pa_stats *stats, uint64_t *unique_reads, uint64_t *ambiguous_reads,
                          uint64_t *first_key, void *stream);
/* Device views for collectives: sum block = [6 stats][G unique][G ambiguous]
 * (reduce with SUM), min block = [G first_key] (reduce with MIN). */
pa_status pa_result_device_view(pa_result *res, uint64_t **sum_block, uint64_t *n_sum, uint64_t **min_block,
                                uint64_t *n_min);
/* Stream-ordered device-to-device copies of the two blocks to / from caller
 * device buffers (e.g. torch tensors reduced with RCCL); either pointer may be
 * NULL.  Values fit int64: counts < 2^63, first keys < 2^63 (PA_NO_FIRST_KEY). */
pa_status pa_result_copy_out(const pa_result *res, void *sum_dst, void *min_dst, void *stream);
pa_status pa_result_copy_in(pa_result *res, const void *sum_src, const void *min_src, void *stream);
/* Overwrite the two blocks from HOST arrays ([6 + 2G] sums, [G] first keys, as
 * pa_result_fetch's order: stats, unique, ambiguous); returns when copied.
 * The host-side reduction of read shards (dumpalign over N GPUs). */
pa_status pa_result_load(pa_result *res, const uint64_t *sum_block, const uint64_t *min_block);
void pa_result_free(pa_result *res);

/* ---- alignment ---------------------------------------------------------------- */

/* Accumulates into `acc`.  read_index_base = global index of reads[0] (orders
 * the Summary keys by first appearance, quirk 9). */
pa_status pa_align(const pa_index *idx, const pa_reads *reads, const pa_params *params, uint64_t read_index_base,
                   pa_result *acc, void *stream);
/* Per-read results.  read_type[n], filtered_kmers[n], redundant_kmers[n],
 * list_off[n+1] (host).  lists may be NULL to query *list_total first. */
pa_status pa_align_detail(const pa_index *idx, const pa_reads *reads, const pa_params *params, uint8_t *read_type,
                          uint32_t *filtered_kmers, uint32_t *redundant_kmers, uint64_t *list_off, uint32_t *lists,
                          uint64_t list_cap, uint64_t *list_total, void *stream);
/* pa_align_detail's outputs, made by the lane kernels for the reads they settle and by
 * the exact kernel for the rest.  Bit for bit pa_align_detail's values.
 * The pass runs once per call.  If list_cap < *list_total the call returns
 * PA_EINVAL with *list_total, read_type, list_off and the two counters valid:
 * the caller retries with the capacity it now knows (lists == NULL behaves as
 * list_cap == 0).  filtered_kmers and redundant_kmers may be NULL.  At most
 * 2^32 - 2 reads per batch (PA_EUNSUPPORTED), as pa_align; PA_EINTERNAL if a
 * read was settled by no kernel (an invariant: never skipped silently).
 * PA_ASSIGN=0 in the environment sends every read to the exact kernel, which is
 * pa_align_detail's pass (A/B runs, a fallback).  DESIGN.md section 11. */
pa_status pa_align_reads(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                         uint8_t *read_type, uint32_t *filtered_kmers /*nullable*/,
                         uint32_t *redundant_kmers /*nullable*/, uint64_t *list_off,
                         uint32_t *lists, uint64_t list_cap, uint64_t *list_total, void *stream);

/* Pairs: mate i of mates1 and mate i of mates2 are one fragment:
 * the pair is classified by the union of both mates' retained k-mers, mate 1's
 * first; no window spans the mates; with min_read_quality a pair is dropped when
 * either mate is.  Per-pair outputs as pa_align_reads gives them per read; acc
 * (nullable) gets the pair counters (first_key = (pair_index_base + i) << 20 |
 * list position), only when the call returns PA_OK.  Any of pair_type / counters
 * may be NULL when only acc is wanted; list_off and lists may then be NULL too.
 * If lists were asked for and list_cap is too small the call returns PA_EINVAL
 * with *list_total, pair_type and list_off valid and acc untouched: the caller
 * retries.  PA_EINVAL when the batches differ in read count or device;
 * PA_EUNSUPPORTED above 2^32 - 2 pairs; PA_EINTERNAL when a pair was settled by
 * no kernel.  *exact_pairs (nullable): pairs the pair-exact kernel classified;
 * the others followed from their mates' results (an unmapped or dropped mate, two
 * ambiguous mates without a specific k-mer).  PA_PAIR_COMBINE=0 in the
 * environment sends every pair that is not dropped to the pair-exact kernel (A/B
 * runs, a fallback); the results are the same. */
pa_status pa_align_pairs(const pa_index *idx, const pa_reads *mates1, const pa_reads *mates2,
                         const pa_params *params, uint64_t pair_index_base, pa_result *acc,
                         uint8_t *pair_type, uint32_t *filtered_kmers, uint32_t *redundant_kmers,
                         uint64_t *list_off, uint32_t *lists, uint64_t list_cap, uint64_t *list_total,
                         uint64_t *exact_pairs, void *stream);
/* ---- coverage: where on a genome its reads fall ----------
 *
 * Every read is classified as pa_align_detail classifies it with the same
 * params.  A uniquely or ambiguously mapped read is placed on each distinct
 * genome g of its list (a p-demoted list holds G* twice: once): every window j
 * of the read whose k-mer w occurs in g's region -- quality and --max-genomes
 * filters or not -- votes for the diagonal min(occ(w, g)) - j; the placement
 * s(read, g) is the diagonal with the most votes, the smallest on a tie.  The
 * read then covers the region positions [s, s + length) inside the region; on a
 * both-strand index (region g + N + reverse complement) position q < |g| is the
 * forward coordinate q, q > |g| is 2|g| - q, the N is dropped, and a read over
 * both halves counts in both.  depth_unique[g][x] / depth_ambiguous[g][x]
 * (uint32, |g| entries, forward coordinates) count the covering reads of each
 * type.  Dropped, unmapped and shorter-than-k reads add nothing.
 *
 * The placements need the k-mers' first occurrence per genome: the positions
 * view of the index, 4 B per table slot + 4 B per (k-mer, genome) pair, built
 * on the device by pa_index_prepare_coverage or by the first pa_coverage_add /
 * pa_align_placements, counted in pa_index_info.device_bytes once it exists,
 * released by pa_index_reduce and pa_index_free.  PA_EUNSUPPORTED for a
 * reference of 2^32 - 1 or more region positions (a both-strand index holds
 * 2|g| + 1 per genome); PA_ENOMEM when it does not fit -- the index then stays
 * usable for everything else.  A coverage job runs on one device. */
typedef struct pa_coverage pa_coverage;
/* Build the positions view now (no-op when it exists); returns when done. */
pa_status pa_index_prepare_coverage(pa_index *idx, void *stream);
/* A zeroed depth accumulator for this index: 8 B per forward genome base on its
 * device.  It serves this index until its next pa_index_reduce (PA_EINVAL
 * after, and for any other index). */
pa_status pa_coverage_create(const pa_index *idx, pa_coverage **out);
pa_status pa_coverage_reset(pa_coverage *cov, void *stream);
/* Classify as pa_align_detail, place, accumulate into `acc` (difference arrays:
 * two atomics per read and genome, four for a read over both halves of a
 * both-strand region).  PA_EUNSUPPORTED when the reads added since
 * the last reset would reach 2^32; PA_EINTERNAL if a listed genome gets no
 * vote (an invariant: never skipped silently).  Returns when done. */
pa_status pa_coverage_add(const pa_index *idx, const pa_reads *reads, const pa_params *params, pa_coverage *acc,
                          void *stream);
/* Per genome (arrays of n_genomes entries, any may be NULL): positions with
 * depth >= min_coverage (>= 1, else PA_EINVAL) and the sum of the depths, for
 * the uniquely and the ambiguously mapped reads. */
pa_status pa_coverage_summary(const pa_coverage *cov, uint32_t min_coverage, uint64_t *covered_unique,
                              uint64_t *covered_ambiguous, uint64_t *sum_unique, uint64_t *sum_ambiguous,
                              void *stream);
/* Depths of positions [first, first + count) of one genome, forward
 * coordinates; either array may be NULL.  PA_EINVAL: genome >= n_genomes, or a
 * range past |g|. */
pa_status pa_coverage_depth(const pa_coverage *cov, uint32_t genome, uint64_t first, uint64_t count,
                            uint32_t *unique_depth, uint32_t *ambiguous_depth, void *stream);
void pa_coverage_free(pa_coverage *cov);
/* pa_align_detail's read_type, list_off and lists, plus starts[i] = s(read,
 * lists[i]) for every list entry (region coordinates, may be negative; the two
 * entries of a p-demoted G* are equal).  lists and starts may both be NULL to
 * query *list_total first. */
pa_status pa_align_placements(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                              uint8_t *read_type, uint64_t *list_off, uint32_t *lists, int64_t *starts,
                              uint64_t list_cap, uint64_t *list_total, void *stream);

/* ---- pileup: what the placed reads say at each position ----
 *
 * Every read is classified as pa_align_detail classifies it with the same
 * params; only PA_UNIQUELY_MAPPED reads (list exactly [g]) contribute.  Such a
 * read is placed as for coverage, s = s(read, g), and piled up only if all of
 * its voting windows vote for s; a read whose windows name two or more
 * diagonals (across a repeat boundary, chimeric) is counted in reads_skipped
 * and adds nothing.  Base i of a piled read lies at region position q = s + i;
 * q outside the region is skipped; on a forward index x = q, b = seq[i]; on a
 * both-strand index q < |g| is x = q, b = seq[i], q == |g| (the N) is skipped,
 * q > |g| is x = 2|g| - q, b = complement(seq[i]).  A base that is not one of
 * A C G T, or whose quality byte < min_base_quality (raw byte, strict, 0
 * filters nothing), is skipped; else count[g][x][b] += 1 (uint32, b = 0-3 for
 * ACGT, x a forward coordinate).
 *
 * Calls: position x of genome g with reference code ref < 4 (forward text) and
 * depth D = the sum of its four counts yields one record per base b != ref, in
 * A, C, G, T order, when D >= min_depth, count[b] >= min_alt_count and
 * 1000 count[b] >= min_alt_permille D (64-bit integers).  Records come ordered
 * by (genome, position, alternative base).  A non-ACGT reference base keeps
 * its counts and is never called.
 *
 * The placements use the positions view (see coverage above; PA_EUNSUPPORTED /
 * PA_ENOMEM as there).  A pileup job runs on one device; the accumulator's
 * bytes are not part of pa_index_info. */
typedef struct pa_pileup pa_pileup;
typedef struct {
    uint64_t reads_piled, reads_skipped, bases_counted;
} pa_pileup_stats;
typedef struct {
    uint32_t genome;
    uint8_t ref, alt, pad[2]; /* codes 0-3 */
    uint64_t position;        /* 0-based, forward */
    uint32_t depth, alt_count;
    uint32_t acgt[4];
} pa_variant;
/* A zeroed accumulator for this index on its device: 16 B of counts per
 * forward genome base, plus its own copy of the forward reference codes (1 B
 * per base), so counts and calls stay readable whatever becomes of the index.
 * It takes reads of this index until its next pa_index_reduce (pa_pileup_add:
 * PA_EINVAL after, and for any other index).  PA_ENOMEM when it does not fit --
 * the index stays usable. */
pa_status pa_pileup_create(const pa_index *idx, pa_pileup **out);
pa_status pa_pileup_reset(pa_pileup *p, void *stream); /* counts and stats to zero */
/* Classify, place and count.  PA_EUNSUPPORTED when the reads added since the
 * last reset would reach 2^32; PA_EINTERNAL if a listed genome gets no vote
 * (an invariant: never skipped silently).  Returns when done. */
pa_status pa_pileup_add(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                        uint32_t min_base_quality, pa_pileup *acc, void *stream);
pa_status pa_pileup_stats_get(const pa_pileup *p, pa_pileup_stats *out, void *stream);
/* Counts of positions [first, first + count) of one genome, forward
 * coordinates: acgt[count][4].  PA_EINVAL: genome >= n_genomes, or a range past |g|. */
pa_status pa_pileup_counts(const pa_pileup *p, uint32_t genome, uint64_t first, uint64_t count,
                           uint32_t *acgt /* [count][4] */, void *stream);
/* The calls.  *n is always the full record count; with cap < *n nothing is
 * written and the call returns PA_EINVAL, so the caller retries with the
 * capacity it now knows (out == NULL behaves as cap == 0).  PA_EINVAL also
 * unless min_depth >= 1, min_alt_count >= 1 and min_alt_permille <= 1000. */
pa_status pa_pileup_variants(const pa_pileup *p, uint32_t min_depth, uint32_t min_alt_count,
                             uint32_t min_alt_permille, pa_variant *out, uint64_t cap, uint64_t *n, void *stream);
void pa_pileup_free(pa_pileup *p);

/* ---- abundance: compatibility classes and an EM over them ----
 *
 * Every read is classified as pa_align_detail classifies it with the same
 * params.  Its compatibility set C(r): none for a dropped, unmapped or
 * shorter-than-k read; {g} for a PA_UNIQUELY_MAPPED read with list [g]; for a
 * PA_AMBIGUOUSLY_MAPPED read (a p-demoted one included) the genomes g with
 * T_r(g) = max_h T_r(h), T_r(g) the number of distinct retained k-mers of the
 * read whose genome set holds g (retained: passed --min-kmer-quality, in the
 * index, passed --max-genomes) -- never empty.  A class is a distinct set C, an
 * ascending genome list, with n_C = its reads; classes are reported sorted
 * lexicographically by genome list, a proper prefix first.  N = sum of n_C.
 *
 * The EM: L_g = |g| - k + 1 (forward windows); theta_g = 1/G for every genome
 * of the index; one iteration is d_C = sum_{g in C} theta_g / L_g, then
 * theta'_g = (1/N) sum_{C holds g} n_C (theta_g / L_g) / d_C (a class with
 * d_C == 0 adds nothing).  max_iterations (1 .. 10000, else PA_EINVAL)
 * iterations run; the loop stops early after one with max_g |theta'_g -
 * theta_g| < tolerance (0: never; negative or NaN: PA_EINVAL).  read_fraction[g]
 * = theta_g, abundance[g] = (theta_g / L_g) / sum_h (theta_h / L_h) (0 when
 * the sum is 0); N == 0 gives zeros and 0 iterations.  All in double precision
 * and without floating-point atomics: the same classes give the same bits,
 * whatever batches the reads came in.
 *
 * The accumulator serves its index until the next pa_index_reduce
 * (pa_abundance_add: PA_EINVAL after, and for any other index); its bytes are
 * not part of pa_index_info.  An abundance job runs on one device. */
typedef struct pa_abundance pa_abundance;
typedef struct {
    uint64_t reads_unique, reads_ambiguous, reads_unmapped, reads_dropped, n_classes, class_entries;
} pa_abundance_info;
pa_status pa_abundance_create(const pa_index *idx, pa_abundance **out);
pa_status pa_abundance_reset(pa_abundance *a, void *stream);
/* Classify, find the ambiguous reads' sets, reduce them to classes on the
 * device (a 64-bit hash of each list, a sort, every list compared with its
 * run's first: a collision is never merged -- the batch is hashed again with
 * another seed, PA_EINTERNAL after three).  Returns when done; after an error
 * `acc` may hold a part of the batch: reset it. */
pa_status pa_abundance_add(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                           pa_abundance *acc, void *stream);
pa_status pa_abundance_info_get(const pa_abundance *a, pa_abundance_info *out, void *stream);
/* class_off[n_classes + 1], genomes[n_entries], counts[n_classes].  *n_classes
 * and *n_entries are always the full sizes; with too small a cap nothing is
 * written and the call returns PA_EINVAL, so the caller retries with the
 * capacities it now knows (NULL arrays behave as caps of 0). */
pa_status pa_abundance_classes(const pa_abundance *a, uint64_t *class_off, uint32_t *genomes, uint64_t *counts,
                               uint64_t cap_classes, uint64_t cap_entries, uint64_t *n_classes, uint64_t *n_entries,
                               void *stream);
/* read_fraction / abundance: n_genomes doubles each; any output may be NULL. */
pa_status pa_abundance_estimate(const pa_abundance *a, uint32_t max_iterations, double tolerance,
                                double *read_fraction, double *abundance, uint32_t *iterations_done,
                                double *last_delta, void *stream);
/* Bootstrap replicates of the estimate.  The classes in
 * reported order are C_0 .. C_{nc-1} with counts n_c, N = sum of n_c, cum_c the
 * exclusive prefix sum of n.  Replicate b (0 <= b < replicates) has key_b =
 * fmix64(seed + 0x9E3779B97F4A7C15 (b + 1)) (mod 2^64; fmix64: MurmurHash3's
 * 64-bit finalizer).  Its draw i (0 <= i < N) is u = fmix64(key_b +
 * 0x9E3779B97F4A7C15 i), r = floor(u N / 2^64), and falls in the class c with
 * cum_c <= r < cum_{c+1}; counts[b][c] is the number of its draws in c, so every
 * row sums to N (integers only: the counts depend on nothing but the classes,
 * the seed and b).  Replicate b's EM is pa_abundance_estimate's, term for term
 * and in its summation order, with counts[b][.] for n_C and the same N, started
 * at 1/G; it stops after its own first iteration with delta < tolerance
 * (iterations[b], last_delta[b]).  read_fraction[b][g] = theta_g of replicate
 * b, abundance[b][g] from it as pa_abundance_estimate computes it.  N == 0
 * gives zeros and 0 iterations.
 *
 * counts: replicates x n_classes (pa_abundance_info_get), read_fraction and
 * abundance: replicates x n_genomes, iterations and last_delta: replicates;
 * row-major; any output may be NULL.  replicates 1 .. 10000, max_iterations and
 * tolerance as pa_abundance_estimate, else PA_EINVAL; PA_ENOMEM when the
 * replicates' device scratch does not fit.  The accumulator is not modified;
 * the call returns when done.  The draws run one workgroup strip per replicate
 * (PA_BOOT_LDS=0 in the environment, read per call, counts through global
 * atomics instead of a histogram in LDS: the same counts), the EMs one
 * workgroup per replicate, every replicate's whole loop in one launch. */
pa_status pa_abundance_bootstrap(const pa_abundance *a, uint32_t replicates, uint64_t seed,
                                 uint32_t max_iterations, double tolerance, uint64_t *counts,
                                 double *read_fraction, double *abundance, uint32_t *iterations,
                                 double *last_delta, void *stream);
void pa_abundance_free(pa_abundance *a);
/* Per read C(r): read_type[n], set_off[n + 1], sets (ascending genomes).  If
 * cap < *total the call returns PA_EINVAL with *total, read_type and set_off
 * valid: the caller retries (sets == NULL behaves as cap == 0), as pa_align_reads. */
pa_status pa_align_candidates(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                              uint8_t *read_type, uint64_t *set_off, uint32_t *sets, uint64_t cap,
                              uint64_t *total, void *stream);

/* ---- lineages: reads and counts rolled up a taxonomy tree ----
 *
 * The tree: nodes 0 .. n_nodes - 1, node 0 the root, parent[0] == 0 and
 * parent[i] < i for i >= 1; genome_node[g], for every genome of the index, is
 * any node (not necessarily a leaf; several genomes may share one).
 *
 * Every read is classified as pa_align_detail classifies it with the same
 * params.  node(r): PA_NO_NODE for a dropped, unmapped or shorter-than-k read;
 * genome_node[g] for a PA_UNIQUELY_MAPPED read with list [g]; for a
 * PA_AMBIGUOUSLY_MAPPED read (a p-demoted one included) the lowest common
 * ancestor of genome_node[g] over g in C(r), the compatibility set
 * pa_align_candidates returns (never empty; not genomes_mapped_to).
 *
 * direct[v] = the reads with node(r) == v; clade[v] = the sum of direct over
 * v's subtree, so clade[0] = the classified reads = unique + ambiguous.  64-bit
 * integers summed with integer atomics only: the same reads give the same
 * counts in whatever batches they come.
 *
 * The library renumbers the nodes in depth-first preorder at creation; the
 * lowest common ancestor of a set is then that of its smallest and its largest
 * preorder number, one climb (a read costs one min/max scan of its set and one
 * climb).  Everything reported is in the caller's node numbers.  direct goes
 * through a histogram in LDS, flushed per workgroup, for trees of up to
 * PA_LINEAGE_LDS_NODES nodes (16 KiB of uint32 counters: eight workgroups of
 * 256 threads per CU, every wave slot, within the 160 KiB of LDS), through
 * 64-bit global atomics above (PA_LINEAGE_LDS=0 in the environment, read per
 * call: global atomics for every tree; the same counts).
 *
 * PA_EINVAL: n_nodes == 0, parent[0] != 0, parent[i] >= i, genome_node[g] >=
 * n_nodes; an accumulator used with another index, or with its own after a
 * pa_index_reduce.  PA_EUNSUPPORTED: more than 2^32 - 2 nodes, reads in a batch
 * or sets in a call.  PA_ENOMEM leaves the index usable.  The accumulator's
 * bytes are not part of pa_index_info; a lineage job runs on one device. */
#define PA_NO_NODE 0xFFFFFFFFu
#define PA_LINEAGE_LDS_NODES 4096
typedef struct pa_lineage pa_lineage;
typedef struct {
    uint64_t reads_unique, reads_ambiguous, reads_unmapped, reads_dropped;
    uint32_t n_nodes, reserved;
} pa_lineage_info;
pa_status pa_lineage_create(const pa_index *idx, const uint32_t *parent, uint32_t n_nodes,
                            const uint32_t *genome_node, pa_lineage **out);
pa_status pa_lineage_reset(pa_lineage *l, void *stream);
/* read_node: host [reads], nullable.  Returns when done; after an error `acc`
 * may hold a part of the batch: reset it. */
pa_status pa_lineage_add(const pa_index *idx, const pa_reads *reads, const pa_params *params, pa_lineage *acc,
                         uint32_t *read_node, void *stream);
/* direct / clade: n_nodes entries each; any output may be NULL. */
pa_status pa_lineage_counts(const pa_lineage *l, uint64_t *direct, uint64_t *clade, pa_lineage_info *info,
                            void *stream);
/* The reduction alone, on the caller's genome sets (a host CSR: set i is
 * sets[set_off[i] .. set_off[i + 1]), set_off ascending from 0): node_out[i] =
 * the lowest common ancestor of genome_node over set i, PA_NO_NODE for an empty
 * set; a genome >= n_genomes or a descending offset is PA_EINVAL.  The
 * accumulator's counts are not touched. */
pa_status pa_lineage_lca(const pa_lineage *l, const uint64_t *set_off, const uint32_t *sets, uint64_t n_sets,
                         uint32_t *node_out, void *stream);
void pa_lineage_free(pa_lineage *l);

/* ---- containment: the distinct reference k-mers the reads hold ----
 *
 * With the pa_params of pa_align (m and p are ignored):
 *   1. A read dropped by --min-read-quality (quality sum < mrq * len, strict) adds
 *      to reads and reads_dropped and to nothing else.
 *   2. Every window j (0 .. len - k) of a kept read, in this order (that of
 *      pa_align's exact kernel, which decides the counters):
 *        a. with --min-kmer-quality: quality sum < mkq * k -> windows_filtered_quality;
 *        b. a base other than ACGT, or a k-mer the index does not hold -> windows_absent;
 *        c. with --max-genomes: set size > mg -> windows_filtered_hr;
 *        d. else the window is retained: windows_retained, seen(w) = 1, and
 *           hits_specific[g] += 1 when its set is {g}.  Repeats within a read and
 *           across reads count every time.
 *      A read shorter than k has no windows.  windows = the sum of the four.
 *   3. Per genome g, S(w) the genome set of k-mer w: kmers[g] = the distinct k-mers
 *      with g in S(w), specific[g] = those with S(w) = {g} (pa_index_extsim_stats'
 *      total and uniq under the identity grouping); kmers_seen[g] and
 *      specific_seen[g] = the same restricted to seen(w) = 1.  On a both-strand
 *      index everything is that of the forward index of the regions T(g).
 *   4. Per node v of a pa_lineage's tree: node(w) = the lowest common ancestor of
 *      genome_node[g] over g in S(w); direct_kmers[v] / direct_seen[v] count the
 *      k-mers with node(w) == v, clade_*[v] are the sums over v's subtree, so
 *      clade_kmers[0] = n_kmers.
 * 64-bit integers made by integer OR and integer add: the same reads give the
 * same numbers in whatever batches they come.
 *
 * The accumulator holds one bit per table slot (capacity / 8 bytes), 8 bytes per
 * genome and eight counters; its bytes are not part of pa_index_info; it runs on
 * one device.  pa_containment_add needs the table and the classes only: an
 * index built with PA_BUILD_DEFER_TILES stays deferred.  hits_specific goes
 * through a histogram in LDS for up to PA_LINEAGE_LDS_NODES genomes, through
 * 64-bit global atomics above (PA_CONTAIN_LDS=0 in the environment, read per
 * call: global atomics always; the same counts).
 *
 * PA_EINVAL: an accumulator used with another index, or with its own after a
 * pa_index_reduce; a lineage made for another index.  PA_ENOMEM leaves the
 * index usable. */
typedef struct pa_containment pa_containment;
typedef struct {
    uint64_t reads, reads_dropped, windows, windows_retained, windows_filtered_quality, windows_filtered_hr,
        windows_absent;
} pa_containment_info;
pa_status pa_containment_create(const pa_index *idx, pa_containment **out);
pa_status pa_containment_reset(pa_containment *c, void *stream);
/* Returns when done; after an error `acc` may hold a part of the batch: reset it. */
pa_status pa_containment_add(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                             pa_containment *acc, void *stream);
/* kmers .. hits_specific: n_genomes entries each; any output may be NULL. */
pa_status pa_containment_counts(const pa_containment *c, uint64_t *kmers, uint64_t *kmers_seen, uint64_t *specific,
                                uint64_t *specific_seen, uint64_t *hits_specific, pa_containment_info *info,
                                void *stream);
/* direct_* / clade_*: the lineage's n_nodes entries each; any output may be NULL. */
pa_status pa_containment_nodes(const pa_containment *c, const pa_lineage *l, uint64_t *direct_kmers,
                               uint64_t *direct_seen, uint64_t *clade_kmers, uint64_t *clade_seen, void *stream);
void pa_containment_free(pa_containment *c);

/* upload + pa_align + fetch for host buffers (stats and per-genome arrays accumulate: +=, min) */
pa_status pa_align_batch(const pa_index *idx, const uint8_t *seq, const uint8_t *qual, const uint64_t *read_off,
                         uint64_t n_reads, uint64_t read_index_base, const pa_params *params, pa_stats *stats,
                         uint64_t *unique_reads, uint64_t *ambiguous_reads, uint64_t *first_key, void *stream);

/* A FASTQ file straight into the align pass (FASTAQFile(path).container +
 * PseudoAlignment.align_reads_from_container, src/data_file.py:134-158,
 * src/records.py:245-302, src/kmer.py:600-620): the host reads the file in
 * windows of window_bytes (0: 128 MiB; threads readers, or zlib for ".gz") into
 * pinned buffers; the DEVICE finds the records, checks them against the
 * grammar, hashes the ids into a duplicate set, packs the read columns and
 * aligns each window while the host reads the next.  Record i of the file is
 * global read read_index_base + i; *n_reads = records.  PA_ENOTCANON: the
 * file is outside the device-parsed subset of the grammar (LF line ends, "+"
 * lines, ids without outer blanks, see csrc/pa_fastq.hip), holds a duplicate
 * id or no record -- `acc` then holds a partial sum: reset it and parse the
 * file the exact way (which also raises the reference's errors). */
pa_status pa_align_fastq_file(const pa_index *idx, const char *path, const pa_params *params,
                              uint64_t read_index_base, pa_result *acc, int32_t threads, uint64_t window_bytes,
                              void *stream, uint64_t *n_reads);

/* pa_align_fastq_file over the byte range [offset, offset + length) of a plain
 * (not gzip) FASTQ file, read as if it were the whole file: the shard of one
 * device in a read-sharded job (the dumpalign CLI with PA_GPUS = N).  The
 * range must start at a record's '@' and end after a record's last line feed
 * (or at the end of the file).  read_index_base orders the shards' records:
 * any base at least as large as the previous shard's base + its record count
 * keeps the Summary key order of one pass over the file (e.g. the range's
 * byte offset: every record takes more than one byte).  ids (nullable): the
 * range's read-id hashes, for pa_idsets_disjoint -- the duplicate-id check
 * (DuplicateRecordError, src/records.py:290-302) across ranges; a duplicate
 * within the range is PA_ENOTCANON as in pa_align_fastq_file. */
typedef struct pa_idset pa_idset;
pa_status pa_align_fastq_range(const pa_index *idx, const char *path, uint64_t offset, uint64_t length,
                               const pa_params *params, uint64_t read_index_base, pa_result *acc, int32_t threads,
                               uint64_t window_bytes, void *stream, uint64_t *n_reads, pa_idset **ids);
/* *disjoint = 1 when no read-id hash is in two of the sets (else 0: a duplicate
 * id across shards, or a 2^-64 hash collision -- parse the file the exact way,
 * which decides and raises the reference's error).  Checked on `device`. */
pa_status pa_idsets_disjoint(const pa_idset *const *sets, uint32_t n_sets, int32_t device, int32_t *disjoint);
void pa_idset_free(pa_idset *ids);

/* Read extraction.  Reads are classified exactly as
 * pa_align_detail classifies them with the same params.  A selection is
 * (type_mask, genome_keep, flags):
 *   type_mask    bits 1u << PA_DROPPED .. 1u << PA_AMBIGUOUSLY_MAPPED; zero or any other bit: PA_EINVAL
 *   genome_keep  NULL, or n_genomes host bytes; restricts MAPPED reads only: a unique or ambiguous
 *                read passes iff its genomes_mapped_to list holds a genome g with genome_keep[g] != 0
 *                (an ambiguous read with an empty list never passes a non-NULL genome_keep); dropped
 *                and unmapped reads are not affected by it
 *   sel(r) = (type_mask has type(r)) && (r is dropped or unmapped, or genome_keep == NULL, or r's list
 *            meets genome_keep), negated when flags & PA_EXTRACT_INVERT. */
#define PA_EXTRACT_INVERT 1u
typedef struct {
    uint32_t type_mask, flags;
    const uint8_t *genome_keep; /* n_genomes bytes or NULL */
} pa_extract_spec;
typedef struct {
    uint64_t records, selected, bytes, selected_by_type[4];
} pa_extract_stats;

/* sel(r) for an uploaded batch: selected[n] host bytes (0 / 1; nullable) and
 * *n_selected.  The kernel-level handle of the selection and the worker of a
 * host-parsed extraction. */
pa_status pa_reads_select(const pa_index *idx, const pa_reads *reads, const pa_params *params,
                          const pa_extract_spec *spec, uint8_t *selected, uint64_t *n_selected, void *stream);

/* pa_align_fastq_file's stream (plain and ".gz"), with the selected records
 * written to out_fd in file order, each as its four lines ending in a line
 * feed ("@" + id, sequence, "+", qualities): for a file inside the
 * device-parsed subset a copy of the record's own bytes, a last record without
 * a final line feed given one.  Per window the device classifies the reads
 * (the assign pass), selects, scans the lengths and gathers the bytes; one
 * copy to pinned memory and one write follow, in window order.  acc
 * (nullable): the counter pass runs on every window as in pa_align_fastq_file.
 * stats: records seen, records selected, bytes written, selected records per
 * type.  PA_ENOTCANON as pa_align_fastq_file gives it, possibly at a late
 * window: the bytes already written stay written and stats->bytes counts them
 * -- truncate the file, reset acc and take the exact path.  PA_EIO: a failed
 * or short write.  PA_EINVAL: a NULL argument or a bad mask.  One device. */
pa_status pa_extract_fastq_file(const pa_index *idx, const char *path, const pa_params *params,
                                const pa_extract_spec *spec, int32_t out_fd, uint64_t read_index_base,
                                pa_result *acc /* nullable */, int32_t threads, uint64_t window_bytes,
                                void *stream, pa_extract_stats *stats);

/* The same as one device-resident step: pa_fastq_prefetch_start begins moving
 * the (plain, not gzip) FASTQ file into device memory on a background thread
 * (parallel positional reads into a pinned ring, copies in file order) and
 * returns at once, so that the copy overlaps the caller's FASTA parse and
 * index build (the dumpalign CLI starts it first); pa_align_fastq_prefetched
 * then parses and aligns the file window by window (window_bytes, 0: 128 MiB)
 * as the bytes land, with the records, errors and PA_ENOTCANON of
 * pa_align_fastq_file.  PA_EUNSUPPORTED for ".gz" paths (use
 * pa_align_fastq_file).  One align per prefetch; free it afterwards. */
typedef struct pa_fastq_prefetch pa_fastq_prefetch;
pa_status pa_fastq_prefetch_start(const char *path, int32_t device, int32_t threads, uint64_t window_bytes,
                                  pa_fastq_prefetch **out);
pa_status pa_align_fastq_prefetched(const pa_index *idx, pa_fastq_prefetch *prefetch, const pa_params *params,
                                    uint64_t read_index_base, pa_result *acc, void *stream, uint64_t *n_reads);
void pa_fastq_prefetch_free(pa_fastq_prefetch *prefetch);

/* The three streams above with every window's reads trimmed on the device
 * (pa_reads_trim's pass) before anything else sees them: the counters, and the
 * selection of an extraction, are those of the trimmed reads.  An extraction
 * still writes the ORIGINAL records, the file's own bytes.  opts NULL, or
 * opts->trim NULL: the plain call.  trim_stats (nullable) ACCUMULATES, the
 * whole file's sums added when the call returns PA_OK and nothing otherwise
 * (PA_ENOTCANON at a late window leaves them as they were).  PA_EINVAL: a spec pa_reads_trim refuses.  One device: pa_align_fastq_range
 * has no trimming form. */
typedef struct {
    const pa_trim_spec *trim;
    pa_trim_stats *trim_stats;
} pa_fastq_opts;
pa_status pa_align_fastq_file_ex(const pa_index *idx, const char *path, const pa_params *params,
                                 uint64_t read_index_base, pa_result *acc, int32_t threads, uint64_t window_bytes,
                                 void *stream, uint64_t *n_reads, const pa_fastq_opts *opts);
pa_status pa_align_fastq_prefetched_ex(const pa_index *idx, pa_fastq_prefetch *prefetch, const pa_params *params,
                                       uint64_t read_index_base, pa_result *acc, void *stream, uint64_t *n_reads,
                                       const pa_fastq_opts *opts);
pa_status pa_extract_fastq_file_ex(const pa_index *idx, const char *path, const pa_params *params,
                                   const pa_extract_spec *spec, int32_t out_fd, uint64_t read_index_base,
                                   pa_result *acc /* nullable */, int32_t threads, uint64_t window_bytes,
                                   void *stream, pa_extract_stats *stats, const pa_fastq_opts *opts);

/* dumpref (KmerReference.get_summary, src/kmer.py:300-329; CLI src/main.py:121-158):
 * the "Kmers" object of the summary written to file descriptor fd as
 * json.dumps(indent=4) text at nesting level 1 ("{" ... "\n    }", or "{}"),
 * from the device index: k-mers in the reference's insertion order (first
 * occurrence in FASTA order), each with its genomes' descriptions and sorted
 * positions.  desc_of[g] numbers genome g's description (desc_json[d]: its
 * JSON string literal, quotes included); genomes sharing a description merge
 * as dict keys do.  keep[g] (NULL: all): genomes left by EXTSIM -- the index
 * must then hold ALL genomes, so that the surviving k-mers keep the full
 * build's order (src/kmer.py:232-245).  Per description: k-mers held by it
 * with one genome / several (unique_kmers / multi_mapping_kmers), its rank of
 * first appearance (the Summary key order; UINT64_MAX if absent) and the last
 * genome met with it (its total_bases); *n_kmers = k-mers written. */
pa_status pa_index_dumpref(const pa_index *idx, const uint8_t *keep, const uint32_t *desc_of, uint32_t n_desc,
                           const char *const *desc_json, int32_t fd, int32_t threads, uint64_t *desc_unique,
                           uint64_t *desc_multi, uint64_t *desc_order, uint32_t *desc_last_genome, uint64_t *n_kmers);

/* Start the HIP runtime and device `device` on a background thread and return
 * at once (a command-line run calls it first, so the runtime's start-up of
 * ~0.15 s overlaps its imports and FASTA parse); later calls wait for it as
 * for any runtime start.  Always PA_OK (errors surface at the first real call). */
pa_status pa_runtime_start(int32_t device);
/* Wait until that start is over (at once when none was made or it is).  A
 * process must not exit while the runtime is still starting on the other
 * thread -- its exit handlers would run under that thread -- so a command-line
 * run calls this on every way out (atexit), the error exits of its flag checks
 * included.  Always PA_OK. */
pa_status pa_runtime_wait(void);

/* ---- multi-GPU reduce (RCCL over xGMI) ------------------------------------------- */

/* One process per GPU, each aligning its own read shard with GLOBAL read
 * indices (read_index_base), then ONE in-place all-reduce of every rank's
 * pa_result: the sum block with ncclSum, the first-key block with ncclMin
 * (uint64).  Afterwards every rank's pa_result holds the job's counters, and
 * pa_result_fetch gives exactly what one process aligning all reads would
 * (Summary key order included).  RCCL is opened at the first call
 * (PA_RCCL_LIBRARY or librccl.so.1); PA_EUNSUPPORTED if it cannot be.
 * `comm` is an ncclComm_t -- from pa_comm_init, or any RCCL communicator of
 * the job's ranks (e.g. the one a framework already made).  Stream-ordered on
 * `stream`; collective: every rank must call it. */
#define PA_COMM_ID_BYTES 128
pa_status pa_comm_unique_id(uint8_t *id /* [PA_COMM_ID_BYTES], rank 0; share it with the others */);
pa_status pa_comm_init(int32_t device, int32_t nranks, int32_t rank, const uint8_t *id, void **comm);
pa_status pa_comm_free(void *comm);
/* ranks in the communicator (ncclCommCount): what a job's reduce really spans */
pa_status pa_comm_count(void *comm, int32_t *nranks);
pa_status pa_counters_reduce(pa_result *res, void *comm, void *stream);

/* ---- profiling ------------------------------------------------------------------ */

/* When enabled, pa_align records HIP events around its main kernel on the
 * stream it launches on; pa_profile_read synchronizes and returns the summed
 * main-kernel milliseconds, launch count, and the reads that took the exact
 * (deferred) path since the last read. */
pa_status pa_profile_enable(pa_index *idx, int32_t enable);
pa_status pa_profile_read(pa_index *idx, double *main_ms, uint64_t *launches, uint64_t *deferred_reads);
/* The same events per kernel of the align pass (each launch bracketed by its
 * own pair on the launch stream): ms[PA_PROF_KERNELS] summed milliseconds and
 * launches[PA_PROF_KERNELS] launch counts since the last call, indexed by
 * PA_PROF_*.  Independent of pa_profile_read (either may be read first). */
#define PA_PROF_QUALITY 0   /* k_quality_masks */
#define PA_PROF_LANE 1      /* k_align_lane (the dominant kernel) */
#define PA_PROF_LANE_NA 2   /* k_align_lane_na */
#define PA_PROF_WAVE 3      /* k_align_fast */
#define PA_PROF_EXACT 4     /* k_align_exact */
#define PA_PROF_LANE_RC 5   /* k_align_lane_rc */
#define PA_PROF_RC_SEEDS 6  /* k_rc_seeds */
#define PA_PROF_KERNELS 7
pa_status pa_profile_read_kernels(pa_index *idx, double *ms, uint64_t *launches);

/* ---- device memory -------------------------------------------------------------- */

/* Buffers of 256 MiB and more (tables, tiles, read columns) come from slabs
 * the library keeps per device and reuses after a free (csrc/pa_mem.cpp: the
 * driver reclaims given-back memory at ~60 GB/s, which stalled rebuilds such as
 * EXTSIM's index of the kept genomes).  pa_mem_trim gives the idle slabs of
 * `device` (-1: every device) back to the driver, for a process that needs the
 * memory elsewhere; *released (may be NULL) = bytes given back.  Allocations
 * that cannot be met otherwise trim by themselves.  No reference counterpart
 * (the reference holds its index in Python dicts). */
pa_status pa_mem_trim(int32_t device, uint64_t *released);

/* ---- ingest (host only, no device) ---------------------------------------------- */

/* Multi-threaded parse of FASTA (kind PA_FASTA) or FASTQ (PA_FASTQ) text into
 * column buffers, for the canonical subset of the reference grammar
 * (src/records.py:141-302; csrc/pa_ingest.cpp states the subset).  Returns
 * PA_ENOTCANON for any text outside it -- including every text the reference
 * rejects (no records, unparsed data, duplicate ids, length mismatch) -- so
 * that the caller parses it with the exact grammar, which reproduces the
 * reference's acceptance and errors.  pa_parse_file reads plain files by mmap
 * and ".gz" files as pa_gz_inflate_file does; PA_EIO if the file cannot be read.
 * A pa_seqset holds n records: FASTA genomes with whitespace removed and
 * stripped descriptions; FASTQ sequences, qualities and stripped ids. */
#define PA_FASTA 0
#define PA_FASTQ 1
typedef struct pa_seqset pa_seqset;
/* universal_newlines: 1 = the text was read from a file in text mode by the
 * reference (CRLF / lone final CR are line breaks), 0 = raw text (parse_records(str)) */
pa_status pa_parse_text(int32_t kind, const char *text, uint64_t len, int32_t threads, int32_t universal_newlines,
                        pa_seqset **out);
pa_status pa_parse_file(int32_t kind, const char *path, int32_t threads, pa_seqset **out);
/* n_bases: total sequence bytes; name_bytes: names joined by '\n' (one after each name) */
pa_status pa_seqset_sizes(const pa_seqset *set, uint64_t *n_records, uint64_t *n_bases, uint64_t *name_bytes);
/* seq[n_bases], qual[n_bases] (FASTQ; may be NULL), off[n_records + 1] (CSR), names[name_bytes] (may be NULL) */
pa_status pa_seqset_export(const pa_seqset *set, uint8_t *seq, uint8_t *qual, uint64_t *off, char *names);
void pa_seqset_free(pa_seqset *set);

/* The text of a ".gz" file, as gzip.open(path).read() returns it
 * (src/data_file.py:123-125), inflated on `threads` host threads: BGZF members
 * in parallel, any other gzip member by chunks whose block boundaries are
 * found by search (csrc/pa_pgz.cpp); every member's CRC-32 and size checked.
 * *n = the text's length; PA_EINVAL if it exceeds cap, PA_ENOTCANON for data
 * gzip.open would not read cleanly (the caller then raises the reference's
 * error through Python's gzip), PA_EIO if the file cannot be opened. */
pa_status pa_gz_inflate_file(const char *path, int32_t threads, uint8_t *dst, uint64_t cap, uint64_t *n);

#ifdef __cplusplus
}
#endif

#endif /* PA_H */
