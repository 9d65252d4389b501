/*
 * drephip.h -- C ABI of libdrephip.so, the MI355X (gfx950) implementation of
 * dRep's primary-clustering hot path: Mash sketch + all-vs-all Mash dist.
 *
 * The reference does this step by shelling out to the external Mash binary
 * (drep/d_cluster.py:481-596, all_vs_all_MASH).  Each entry point below names
 * the reference interface it replaces.  Conventions:
 *   - every function returns 0 on success and a negative DREPHIP_ERR_* code on
 *     failure (the reference ignored mash's exit codes, drep/__init__.py:44-48;
 *     here failures are reported) -- drephip_last_error() gives the message
 *     (thread-local);
 *   - host buffers are owned by the caller (numpy arrays via ctypes); device
 *     memory passed in (d_ prefix) is owned by the caller too; the library owns
 *     its own device scratch, kept in the context;
 *   - calls are blocking and a context is single-caller; no C++ exception
 *     crosses the ABI.
 *
 * Sketch definition (bit-exact with `mash sketch -k 21 -s S`, seed 42):
 *   canonical k-mer (memcmp(fwd, revcomp) <= 0 ? fwd : revcomp) hashed with
 *   MurmurHash3_x64_128(seed).h1 over its ASCII bytes; k-mers containing a
 *   non-ACGT byte (after upper-casing) or spanning two records are skipped;
 *   sketch = the s smallest distinct hashes, ascending, one sketch per file.
 * hashes_out rows are s wide; entries past nhash are UINT64_MAX.
 *
 * Pair output: condensed upper triangle (i < j, row-major; scipy squareform
 * order): index(i, j) = i*N - i*(i+1)/2 + (j - i - 1).
 *   common = Mash's shared-hash count (the "c" of "c/denom" in MASH_table.tsv),
 *   denom  = s when both sketches are full, else min(s, |A u B|).
 */
#ifndef DREPHIP_H
#define DREPHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DREPHIP_OK               0
#define DREPHIP_ERR_ARG         -1
#define DREPHIP_ERR_HIP         -2
#define DREPHIP_ERR_IO          -3
#define DREPHIP_ERR_NOMEM       -4
#define DREPHIP_ERR_UNSUPPORTED -5
#define DREPHIP_ERR_INTERNAL    -6

typedef struct drephip_ctx drephip_ctx;

/* Library/ABI version (major*10000 + minor*100 + patch). */
int drephip_version(void);

/* Build identity: "src=<sha256 of the library's sources>;arch=gfx950;extra=<A/B
 * build flags>" -- the digest is computed by drep_amd/csrc/Makefile over
 * include/drephip.h and drep_amd/csrc/ (drep_amd/_lib.py:source_digest restates
 * it), so a caller can prove which sources the loaded library was built from. */
const char *drephip_build_id(void);

/* Last error message of the calling thread ("" if none). */
const char *drephip_last_error(void);

/* Number of visible HIP devices. */
int drephip_device_count(int *n);

/* Create a context on HIP device `device` for k-mer size k (1..32), sketch
 * size s (1..DREPHIP_MAX_SKETCH) and Murmur seed.
 * Replaces: the `mash` executable lookup + parameters,
 *   drep/d_cluster.py:499-515 (MASH_sketch, exe_loc/get_exe), drep/__init__.py:88-101. */
int drephip_create(int device, int k, uint32_t s, uint32_t seed, drephip_ctx **out);
int drephip_destroy(drephip_ctx *ctx);

/* Largest supported sketch size. */
uint32_t drephip_max_sketch(void);

/* ---------------------------------------------------------------- layout
 * Packed genome set in HBM: 2-bit base codes (A0 C1 G2 T3), 16 bases per
 * uint32 (base p at bits 2*(p%16)); validity bitmap, 32 bases per uint32 (bit
 * p%32 of word p/32).  Genome g occupies bases [base_off[g], base_off[g] +
 * padded[g]); base_off[0] = tile, base_off and padded are multiples of
 * drephip_tile_bases(); records are separated by one invalid base and every
 * genome is followed by at least one invalid base; bases [0, tile) are
 * invalid. */
uint64_t drephip_tile_bases(void);

/* Padded size (in bases) of a genome whose records have the given lengths. */
uint64_t drephip_padded_bases(const uint64_t *rec_len, uint32_t n_rec);

/* Parse a FASTA file (plain or gzip; kseq semantics as in Mash) -- what
 * `mash sketch <fasta>` reads (drep/d_cluster.py:543-544).  Outputs the sum of
 * record lengths, the padded size, the record count and the number of valid
 * k-mer positions. */
int drephip_fasta_info(const char *path, int k, uint64_t *length, uint64_t *padded,
                       uint32_t *n_records, uint64_t *n_kmers);

/* Pack a FASTA into the layout at base offset `base_off` of caller-owned host
 * arrays (codes/valid sized for at least base_off+padded bases; the genome's
 * padded region must be zero on entry). */
int drephip_fasta_pack(const char *path, int k, uint32_t *codes, uint32_t *valid,
                       uint64_t base_off, uint64_t cap_bases, uint64_t *length,
                       uint64_t *n_kmers);

/* ---------------------------------------------------------------- sketch
 * Replaces: `mash sketch <fa> -s S -o <out>` per genome on a thread pool
 * (drep/d_cluster.py:531-549, drep/__init__.py:53-59) and `mash paste`
 * (d_cluster.py:551-567): one call sketches a whole genome set into one
 * row-major uint64[n_genomes][s] matrix.
 * Input: concatenated sequence bytes (any case) of every record of every
 * genome; rec_off[n_rec+1] record boundaries into seq; genome g owns records
 * [genome_rec_off[g], genome_rec_off[g+1]). */
int drephip_sketch(drephip_ctx *ctx, const uint8_t *seq, const uint64_t *rec_off, uint32_t n_rec,
                   const uint64_t *genome_rec_off, uint32_t n_genomes,
                   uint64_t *hashes_out, uint32_t *nhash_out, uint64_t *length_out);

/* Same, reading FASTA files (kseq semantics, plain or gzip) on `threads` CPU
 * threads (0 = all).  Files are read and packed in batches of ~1 Gbase into
 * two pinned host buffers by a producer thread while the calling thread copies
 * the previous batch to the device and sketches it (host ingest and GPU work
 * overlap).  drephip_last_ingest_stats reports the split. */
int drephip_sketch_files(drephip_ctx *ctx, const char *const *paths, uint32_t n_genomes,
                         int threads, uint64_t *hashes_out, uint32_t *nhash_out,
                         uint64_t *length_out);

/* Timing of the last drephip_sketch_files call on this context (seconds):
 * host read + pack summed over batches, device copy + sketch summed over
 * batches, the whole call's wall time, and the number of batches.  With the
 * overlap, wall ~ produce + the last batch's device work. */
int drephip_last_ingest_stats(drephip_ctx *ctx, double *produce_s, double *gpu_s, double *wall_s,
                              uint32_t *batches);

/* Host phases of the last drephip_sketch_files call, summed over the worker
 * threads (seconds): FASTA read + parse (gzip inflate included) and the 2-bit
 * pack; and the number of genomes whose span outgrew the region their file
 * size (or gzip ISIZE) reserved, repacked at the end of their batch. */
int drephip_last_ingest_phases(drephip_ctx *ctx, double *read_thread_s, double *pack_thread_s,
                               uint32_t *overflow);

/* ---------------------------------------------------------------- device ingest
 * The kseq parse, the 2-bit pack and the validity bitmap done by kernels on
 * FASTA text that is already in device memory; bit-exact with
 * drephip_fasta_pack for every file that holds no FASTQ record.
 *
 * Text tile: the kernels cut each file into pieces of this many bytes (a
 * power of two); exposed so that tests can aim at its edges. */
uint32_t drephip_text_tile_bytes(void);

/* Device-memory form of drephip_fasta_pack for n_files files at once -- the
 * same `mash sketch <fasta>` read (drep/d_cluster.py:543-544).  d_text holds
 * the files' plain text, every file starting on a 16-byte boundary: file f
 * ends at byte h_text_off[f+1] and starts at the 16-byte boundary at or after
 * h_text_off[f] (the end of the file before it), so the up to 15 bytes between
 * two files belong to no file and are never read as text.  d_text and
 * h_text_off[0] must be 16-byte aligned and h_text_off non-decreasing
 * (DREPHIP_ERR_ARG otherwise); nothing at or past h_text_off[n_files] is read.
 * Genome f is packed at base
 * h_base_off[f] of d_codes/d_valid into a region of h_cap_bases[f] bases, both
 * multiples of drephip_tile_bases(); the call zeroes each region itself.  A
 * region of drephip_padded_bases of ONE record as long as the file's text
 * always suffices.  Per file (host arrays of n_files entries, each nullable):
 * length (sequence bytes), padded span, record count, valid k-mer positions
 * for the context's k, and status: 0 packed; 1 the file holds a record line
 * starting with '+' (FASTQ) and needs the host reader, nothing was packed;
 * 2 the region is too small, nothing was written.  Nothing outside a file's
 * region is ever written.  Runs on `stream`; blocking. */
int drephip_fasta_pack_device(drephip_ctx *ctx, const uint8_t *d_text, const uint64_t *h_text_off,
                              uint32_t n_files, const uint64_t *h_base_off, const uint64_t *h_cap_bases,
                              uint32_t *d_codes, uint32_t *d_valid, uint64_t *length_out, uint64_t *padded_out,
                              uint32_t *n_records_out, uint64_t *n_kmers_out, uint8_t *status_out, void *stream);

/* Who parses and packs the files of drephip_sketch_files.  HOST (the default):
 * worker threads, as described above.  DEVICE: the workers only read each
 * plain file's bytes into pinned memory; the text is copied to the device,
 * packed there (drephip_fasta_pack_device) and sketched in place.  gzip files
 * and files with FASTQ records still take the host reader, file by file.  The
 * results are identical.  A new context takes its path from the environment
 * variable DREPHIP_INGEST=host|device when it is set.  On the DEVICE path
 * drephip_last_ingest_stats / _phases keep their meaning: read_thread_s is the
 * raw read (plus the host reader's share for gzip and FASTQ files),
 * pack_thread_s counts only the files the host packed, and gpu_s includes the
 * text copy and the pack kernels. */
#define DREPHIP_INGEST_HOST   0
#define DREPHIP_INGEST_DEVICE 1
int drephip_set_ingest_path(drephip_ctx *ctx, int path);
int drephip_get_ingest_path(drephip_ctx *ctx, int *path);

/* The last drephip_sketch_files call: files packed on the device, files that
 * took the host reader, and bytes of text copied to the device (0, n, 0 after
 * a HOST-path call). */
int drephip_last_ingest_paths(drephip_ctx *ctx, uint32_t *device_files, uint32_t *host_files,
                              uint64_t *text_bytes);

/* Device-resident sketch: packed genome set already in HBM (see layout).
 * h_base_off/h_padded/h_nkmers are host arrays of n_genomes entries
 * (h_nkmers: valid k-mer positions, used only to seed the candidate
 * threshold).  d_hashes: uint64[n_genomes][s]; d_nhash: uint32[n_genomes].
 * stream: a hipStream_t; 0 is the HIP null stream (as everywhere in HIP).
 * Every device-pointer entry point runs on the stream it is given, so it is
 * ordered after work the caller queued there.  Blocking. */
int drephip_sketch_device(drephip_ctx *ctx, const uint32_t *d_codes, const uint32_t *d_valid,
                          const uint64_t *h_base_off, const uint64_t *h_padded,
                          const uint64_t *h_nkmers, uint32_t n_genomes,
                          uint64_t *d_hashes, uint32_t *d_nhash, void *stream);

/* Same as drephip_sketch_device, but returns once the first threshold round
 * is queued, without waiting for it: work the caller queues next on `stream`
 * (the sketch all-gather, drephip_allpairs_device) runs right behind it.
 * d_hashes/d_nhash are final only after drephip_sketch_wait, which must be
 * called before the next sketch call on this context: until then every other
 * sketch call fails with DREPHIP_ERR_ARG (the pending check is kept).  The
 * inputs (d_codes, d_valid) must stay unchanged until the wait, which may
 * rerun the call from them. */
int drephip_sketch_device_async(drephip_ctx *ctx, const uint32_t *d_codes, const uint32_t *d_valid,
                                const uint64_t *h_base_off, const uint64_t *h_padded,
                                const uint64_t *h_nkmers, uint32_t n_genomes,
                                uint64_t *d_hashes, uint32_t *d_nhash, void *stream);

/* Completes a drephip_sketch_device_async call: waits for its stream, checks
 * every genome's first-round status and, if any genome needs another
 * threshold round (a genome with fewer distinct k-mers than expected, or
 * heavy repeats), reruns the whole call synchronously and sets *redone = 1:
 * anything the caller computed from the sketches in between must then be
 * recomputed.  *redone = 0 otherwise (also when nothing is pending).  The
 * sketch kernels' drephip_last_kernel_ms entries (0, 1) are set here. */
int drephip_sketch_wait(drephip_ctx *ctx, int *redone);

/* Bench/test input: write synthetic genomes g0..g0+n-1 (each length L, one
 * record; family = g / family_size) into the packed layout with
 * genome i at base_off = tile + i*drephip_padded_bases(&L, 1).
 * d_codes/d_valid must hold tile + n*padded bases. */
int drephip_synth_device(drephip_ctx *ctx, uint64_t seed, uint32_t g0, uint32_t n,
                         uint32_t family_size, uint64_t L, uint32_t *d_codes, uint32_t *d_valid,
                         void *stream);

/* The sketch hash kernel's reject-early test, evaluated on the host through the
 * inline functions the kernel calls (drep_amd/csrc/prefilter.h; no context, no
 * GPU).  A k-mer reaches the test as the two fmix64 states before their last
 * multiply, (q1, q2); its hash is h1 = fin(q1 C2) + fin(q2 C2), fin(p) =
 * p ^ (p >> 33).  For each of the n pairs and the threshold T: pass[i] = the
 * prefilter lets the k-mer through to the exact test, exact[i] = h1 <= T.
 * The prefilter is a necessary condition: exact implies pass. */
int drephip_prefilter_eval(const uint64_t *q1, const uint64_t *q2, uint64_t n, uint64_t T,
                           uint8_t *pass, uint8_t *exact);

/* The sketch hash kernel's canonical-strand choice, evaluated on the host
 * through the inline functions the kernel calls (drep_amd/csrc/canon.h; no
 * context, no GPU).  words holds n triples of 2-bit code words F[m-2], F[m-1],
 * F[m] (word j = bases 16j..16j+15, base i at bits 2i; A, C, G, T = 0..3), and
 * r (0..15) names the window end q = 16m + r, the 21-mer of bases q-20..q.
 * For each triple: hi[i] = bases 0-15 of the canonical k-mer (the smaller of
 * the k-mer and its reverse complement in ASCII order), base 0 in the top two
 * bits; tail[i] = its bases 16-20 as a 10-bit number, base 16 on top.  The
 * kernel indexes its tail table by the top five bases of the other strand's
 * high word; the natural index returned here is that index taken through
 * tail_index_of_head, the map the table is stored by. */
int drephip_canon_eval(const uint32_t *words, uint64_t n, uint32_t r, uint32_t *hi, uint32_t *tail);

/* ---------------------------------------------------------------- dist
 * Replaces: `mash dist -p P ALL.msh ALL.msh > MASH_table.tsv`
 * (drep/d_cluster.py:569-573) for the integer part of every row: the shared-
 * hash count and its denominator.  Distances are a pure function of
 * (common, denom) and are formed on the host (drephip_distance_lut).
 * Input: N rows of s hashes, ascending and distinct; entries past nhash[i] are
 * UINT64_MAX (as drephip_sketch* write them -- the kernels read whole rows).
 * drephip_allpairs and drephip_allpairs_rows check nhash[i] <= s and the
 * UINT64_MAX padding, but not that a row ascends: an unordered row is
 * accepted and its counts mean nothing.  Every other host form checks all
 * three; the device entry points assume them. */
int drephip_allpairs(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                     uint16_t *common_out, uint16_t *denom_out /* nullable */);

/* drephip_allpairs restricted to rows [row0, row1) of the upper triangle
 * (columns row+1..N-1): common_out/denom_out receive the condensed segment
 * that starts at index(row0, row0+1), i.e. row0*N - row0*(row0+1)/2.  One call
 * per device (one context each) splits the triangle across GPUs inside one
 * process -- the multi-device form of the same `mash dist` step. */
int drephip_allpairs_rows(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                          uint32_t row0, uint32_t row1, uint16_t *common_out, uint16_t *denom_out /* nullable */);

/* Device-resident all-pairs over rows [row0, row1) of the upper triangle
 * (columns row+1..N-1).  d_common/d_denom receive the condensed segment that
 * starts at index(row0, row0+1).  d_denom may be NULL. Blocking. */
int drephip_allpairs_device(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                            uint32_t N, uint32_t row0, uint32_t row1, uint16_t *d_common,
                            uint16_t *d_denom, void *stream);

/* Same as drephip_allpairs_device, but on the whole-row table path (s <=
 * 2048) it returns once the kernels are queued: the host can queue the next
 * step's work while they run.  The output is final once the work queued on
 * `stream` before and by this call has run (the kernels handle every row
 * themselves, including a row whose table cannot be built, which they merge
 * literally); drephip_allpairs_wait (or any later all-pairs or linkage call on
 * this context) waits for it.  Other paths run synchronously (the wait is
 * then a no-op).  Kernel timings of a deferred call are not recorded. */
int drephip_allpairs_device_async(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                  uint32_t N, uint32_t row0, uint32_t row1, uint16_t *d_common,
                                  uint16_t *d_denom, void *stream);
int drephip_allpairs_wait(drephip_ctx *ctx);

/* Reference all-pairs kernel (one lane per pair, literal Mash merge loop).
 * Same contract as drephip_allpairs_device; slower; used for cross-checks. */
int drephip_allpairs_merge_device(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                  uint32_t N, uint32_t row0, uint32_t row1, uint16_t *d_common,
                                  uint16_t *d_denom, void *stream);

/* Mash distance for common = 0..denom at the given denominator (host, libm):
 * J = c/denom; d = c==denom ? 0 : c==0 ? 1 : min(1, -ln(2J/(1+J))/k).
 * Reference: the "dist" column of MASH_table.tsv parsed at d_cluster.py:581. */
int drephip_distance_lut(int k, uint32_t denom, double *lut /* denom+1 */);

/* MASH_table.tsv as `mash dist -p P ALL.msh ALL.msh > MASH_table.tsv` prints
 * it (drep/d_cluster.py:569-573): for every query q (outer loop) and reference
 * r, "names[r]\tnames[q]\t%g dist\t%g p-value\tcommon/denom\n".  Pairs come
 * from the condensed result (index(i, j), i < j; denom NULL = s for every
 * pair) with their distances and p-values (caller-computed: Mash's formula,
 * drephip_distance_lut; p-values with the binomial tail); a genome against
 * itself prints distance 0, self_pval[q] and self_count[q]/self_count[q].
 * Host only; rows are formatted on `threads` threads (0 = all) and written in
 * order. */
int drephip_write_mash_table(const char *path, const char *const *names, uint32_t N,
                             const uint16_t *common, const uint16_t *denom /* nullable */, uint32_t s,
                             const double *dist, const double *pval, const uint16_t *self_count,
                             const double *self_pval, int threads);

/* All-pairs kernel selection (no CPU path exists; every choice is a HIP kernel
 * with the same bit-exact result):
 *   DREPHIP_AP_AUTO  whole-row LDS tables for s <= 2048, value bands above;
 *   DREPHIP_AP_TABLE k_allpairs_q (s <= 2048);
 *   DREPHIP_AP_BAND  k_allpairs_band, band_cap (1..1024) elements per row per
 *                    band, clamped to the kernel's LDS budget (768; the
 *                    default is the production setting; small caps exercise
 *                    many bands on small sketches in tests);
 *   DREPHIP_AP_MERGE k_allpairs_merge (literal merge, cross-check only). */
#define DREPHIP_AP_AUTO 0
#define DREPHIP_AP_TABLE 1
#define DREPHIP_AP_BAND 2
#define DREPHIP_AP_MERGE 3
int drephip_set_allpairs_path(drephip_ctx *ctx, int path, uint32_t band_cap);

/* The shared-hash screen in front of the table / band kernels (an exact
 * shortcut inside `mash dist`, drep/d_cluster.py:569-573): Mash's merge of two
 * sketches that share no hash is common 0, denominator min(s, |A| + |B|), so
 * the sketch entries are grouped by value (radix sort on the device), the
 * (row tile, column) cells whose genomes share a hash are listed, the kernels
 * run on those only and every other pair is written as no-shared-hash.
 *   DREPHIP_SCREEN_AUTO  on when N >= 4096 and the pair checks the grouping
 *                        implies stay below (pairs x s) / 16 (else the dense
 *                        item plan runs);
 *   DREPHIP_SCREEN_ON    always (unless N x s >= 2^32);
 *   DREPHIP_SCREEN_OFF   never.
 * The environment variable DREPHIP_AP_SCREEN (0/1/2) overrides the mode. */
#define DREPHIP_SCREEN_AUTO 0
#define DREPHIP_SCREEN_ON 1
#define DREPHIP_SCREEN_OFF 2
int drephip_set_allpairs_screen(drephip_ctx *ctx, int mode);
/* The last all-pairs call's screen: whether it replaced the dense plan, the
 * sketch entries grouped, the runs of equal keys, the pair checks, the
 * marked (row tile, column) cells left to the kernels and the pairs sharing
 * exactly one hash that the screen wrote itself.  After
 * drephip_allpairs_device_marked: entries, runs and checks of the hash part
 * this context grouped last. */
int drephip_last_screen_stats(drephip_ctx *ctx, int *used, uint64_t *entries, uint64_t *runs, uint64_t *checks,
                              uint64_t *marked, uint64_t *simple);

/* The sharded screen (a W-way sharded `mash dist`, one rank per GPU): instead
 * of every rank grouping all N x s entries, rank p groups hash part p of W
 * (the p-th of W hash value ranges, cut at the medians over the genomes of
 * each sketch's p/W quantiles, so every rank computes the same cuts: equal
 * hashes lie in one part, and each sketch row -- ascending, as every all-pairs
 * call requires -- holds a part's hashes in one range), marks the (row tile, column) cells of EVERY
 * row from its runs of >= 3 and lists its runs of two; the ranks route the
 * marks to the ranks owning their rows (an all-to-all: RCCL or gloo, the
 * caller's), and each rank screens its own rows from what it received.  Same
 * result as drephip_allpairs_device with the screen on (no light cells).
 * Replaces the per-rank grouping inside the sharded form of
 * drep/d_cluster.py:569-573.
 *
 * drephip_screen_geometry: rows per row tile R (the all-pairs kernels' for
 * this s).  Row tiles count from row 0: tile T holds rows [T R, (T + 1) R).
 * drephip_screen_part: part `part` of `nparts`; *checks = the part's pair
 * checks (their sum over the parts decides the screen: drephip_screen_worth
 * sets *applies when this context screens N genomes at all -- mode, N, N x s --
 * and *use when it would screen them with those checks, as
 * drephip_allpairs_device decides), *n_cells = its marked cell words,
 * *n_records = its runs-of-two records.  The part's bitmap of every row is
 * walked in blocks of row tiles (an eighth of the free device memory per
 * block; DREPHIP_SCREEN_PART_BLOCK_TILES sets the tiles per block, tests): the
 * cells come out in the same order whatever the blocks.  Blocking.  Results stay in the
 * context until drephip_screen_part_copy copies them out, each as 4 uint32:
 *   cell   {T, w, bits, 0}: columns 32 w + b (bit b set) of row tile T marked
 *   record {a, b, (i << 16) | j, 0}: genomes a < b hold one hash at positions
 *          i, j (a run of two);
 * route a cell to the rank owning rows T R.., a record to the rank owning row a.
 * drephip_allpairs_device_marked: drephip_allpairs_device over rows
 * [row0, row1) screened from the cells and records given (every part's for
 * these rows; others are ignored).  Rank boundaries on multiples of R keep the
 * marks exact; otherwise a tile straddling a boundary gives both ranks its
 * cells (more kernel work, the same result). */
int drephip_screen_geometry(drephip_ctx *ctx, uint32_t *rows_per_tile);
int drephip_screen_part(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash, uint32_t N,
                        uint32_t part, uint32_t nparts, uint64_t *checks, uint32_t *n_cells, uint32_t *n_records,
                        void *stream);
int drephip_screen_part_copy(drephip_ctx *ctx, uint32_t *d_cells, uint32_t *d_records, void *stream);
int drephip_screen_worth(drephip_ctx *ctx, uint32_t N, uint64_t checks, int *applies /* nullable */, int *use);
int drephip_allpairs_device_marked(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash, uint32_t N,
                                   uint32_t row0, uint32_t row1, uint16_t *d_common, uint16_t *d_denom,
                                   const uint32_t *d_cells, uint64_t n_cells, const uint32_t *d_records,
                                   uint64_t n_records, void *stream);

/* ------------------------------------------------------------ sparse all-pairs
 * `mash dist` (drep/d_cluster.py:569-573) over rows [row0,row1) of the upper
 * triangle, listing only the pairs that share a hash: no condensed vector of
 * N(N-1)/2 entries is written, so N is not bounded by N^2 bytes.  A record is
 * 4 uint32 {i, j, common, denom}, i < j (genome indices as given), common > 0,
 * denom as in the condensed output (always filled); a pair that is not listed
 * has common 0, i.e. Mash distance 1.  Every unordered pair appears at most
 * once; the order of the records is unspecified.
 *
 * The caller provides room for `cap` records.  When the rows hold more, the
 * call stores the first `cap` reserved slots only (nothing outside [0, cap)),
 * returns DREPHIP_ERR_NOMEM and sets *n_pairs to the number needed, so one
 * retry with that size succeeds; cap = 0 (pairs may be NULL) only counts.
 *
 * Plans: with the whole-row tables (s <= 2048) and the shared-hash screen in
 * use (DREPHIP_SCREEN_ON, or DREPHIP_SCREEN_AUTO from 4096 genomes on unless
 * the set is dense) the screen and the LIST kernel append their non-zero pairs
 * themselves, walking the rows in blocks so that the screen's scratch stays
 * inside a budget taken from the device's free memory.  Every other plan (band
 * path, screen off or dense, N x s >= 2^32, DREPHIP_AP_MERGE) computes a
 * temporary condensed segment of at most 2^28 pairs per row block inside the
 * context and compacts its non-zero counts.  The environment variable
 * DREPHIP_SPARSE_BLOCK_ROWS sets the rows per block of either plan (tests).
 * drephip_last_screen_stats and drephip_last_kernel_ms describe the call's
 * screen and kernels as after drephip_allpairs_device.  Blocking. */
int drephip_allpairs_sparse_device(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                   uint32_t N, uint32_t row0, uint32_t row1,
                                   uint32_t *d_pairs /* cap x 4 */, uint64_t cap, uint64_t *n_pairs, void *stream);
/* The sharded form: drephip_allpairs_sparse_device over rows [row0, row1)
 * screened from the cells and records given -- every hash part's marks of the
 * sharded screen (drephip_screen_part, routed as for
 * drephip_allpairs_device_marked); marks of other rows are ignored.  The
 * record contract is the one above; a pair belongs to the call that owns its
 * smaller genome, so the lists of disjoint row ranges never share a pair and
 * those of a partition of [0, N) together are the whole list.
 *
 * With the whole-row tables (s <= 2048) the rows are walked in blocks as
 * above (a multiple of R rows, the same budget, DREPHIP_SPARSE_BLOCK_ROWS);
 * per block the cells are clipped to its rows, the pair map is built from the
 * records of its rows, and every pair has one writer: a pair held by a single
 * run of two, both sketches full, in an unmarked cell is appended by the
 * screen (common 1 when its rank sum is below s, else nothing); every other
 * pair -- two runs of two (one per hash part), a partial sketch, a cell a
 * longer run of any part marked -- goes to the LIST kernel.  No light cells.
 * A tile that straddles row0, row1 or a block edge gets a superset of marks
 * and still emits only the rows it owns.  The band path (s > 2048) and a block
 * whose pair map or lists outgrow the screen's limits run
 * drephip_allpairs_device_marked into the temporary segment and compact it.
 * Errors as drephip_allpairs_device_marked: DREPHIP_ERR_ARG for null pointers
 * and DREPHIP_AP_MERGE, DREPHIP_ERR_UNSUPPORTED for N x s >= 2^32; and
 * DREPHIP_ERR_NOMEM as above.  Stats as after drephip_allpairs_sparse_device
 * (entries, runs and checks: the hash part this context grouped last). */
int drephip_allpairs_sparse_device_marked(drephip_ctx *ctx, const uint64_t *d_hashes, const uint32_t *d_nhash,
                                          uint32_t N, uint32_t row0, uint32_t row1,
                                          const uint32_t *d_cells, uint64_t n_cells,
                                          const uint32_t *d_records, uint64_t n_records,
                                          uint32_t *d_pairs /* cap x 4 */, uint64_t cap, uint64_t *n_pairs,
                                          void *stream);
/* The host form: sketches checked as drephip_allpairs requires them (rows
 * ascending and distinct, UINT64_MAX past nhash[i]; DREPHIP_ERR_ARG otherwise). */
int drephip_allpairs_sparse(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                            uint32_t row0, uint32_t row1, uint32_t *pairs /* cap x 4 */, uint64_t cap,
                            uint64_t *n_pairs);
/* last sparse call: row blocks walked, pairs from the direct kernels, pairs from the
 * fallback compaction, peak bytes of context scratch */
int drephip_last_sparse_stats(drephip_ctx *ctx, uint32_t *blocks, uint64_t *direct, uint64_t *fallback,
                              uint64_t *scratch_bytes);

/* ------------------------------------------------- query against reference
 * Replaces: `mash dist <reference.msh> <query.msh>`, the two-file form of the
 * call at drep/d_cluster.py:569-573 (which passes ALL.msh twice): Q query
 * sketches against N reference sketches, both matrices of s hashes per row as
 * the dist section above requires them.  The result is the Q x N rectangle of
 * (common, denom), defined as in that section: denominator s when both
 * sketches are full, else min(s, |A u B|).  There is no diagonal: a query that
 * is also a reference meets itself (common = denom = its hash count; 0 / 0 for
 * two empty sketches), as the self rows of Mash's table do.
 *
 * drephip_dist_rect_device: rows [q0, q1) of the rectangle (q1 clamped to Q);
 * d_common / d_denom hold (q1 - q0) x N entries, row-major -- pair (q, r) at
 * (q - q0) * N + r -- and nothing else is written; d_denom may be NULL.
 * Q == 0, N == 0 or q0 >= q1: DREPHIP_OK, nothing written.  Null pointers:
 * DREPHIP_ERR_ARG.  Kernels: the RECT flavour of k_allpairs_q (whole-row LDS
 * tables of the query rows, the reference sketches streamed as columns) for
 * s <= 2048 (DREPHIP_AP_AUTO / DREPHIP_AP_TABLE); above, under
 * DREPHIP_AP_AUTO, the RECT flavour of k_allpairs_band (value bands of the
 * query rows: R = 4, 2^11 slots, at most 768 elements per row per band, 128
 * reference columns per item; no value rounds), which reruns the call's rows
 * by k_rect_merge when a band table cannot be built; k_rect_merge (the
 * literal merge, one lane per pair) for DREPHIP_AP_MERGE and, above 2048, for
 * DREPHIP_RECT_BAND_OFF (drephip_set_rect_band below).  A context set to
 * DREPHIP_AP_BAND, the triangle's selector, gets DREPHIP_ERR_UNSUPPORTED.  The
 * two-set shared-hash screen (drephip_set_rect_screen below) may run in front
 * of the table and band kernels, never in front of k_rect_merge.  Blocking, on the caller's stream; a pending
 * drephip_allpairs_device_async on the context is waited for first.
 * drephip_last_kernel_ms `which` 2 / 3 report the rectangle's kernel (the
 * rerun included) and its table build.  With DREPHIP_DEBUG set the band route
 * prints one line per call (per row block of the record and best-hit forms):
 * "[drephip] rect band plan: R 4 C 128 cap .. items .. slots .. pieces .."
 * (elements per row per band, (row tile, column tile) pairs, item slots with
 * the idle ones, kernel dispatches).  The device forms assume well-formed
 * rows. */
int drephip_dist_rect_device(drephip_ctx *ctx, const uint64_t *d_qhashes, const uint32_t *d_qnhash, uint32_t Q,
                             const uint64_t *d_rhashes, const uint32_t *d_rnhash, uint32_t N, uint32_t q0,
                             uint32_t q1, uint16_t *d_common, uint16_t *d_denom /* nullable */, void *stream);
/* The rectangle's band kernel (s > 2048 under DREPHIP_AP_AUTO).  band_cap:
 * elements per row per band, 1..1024 (else DREPHIP_ERR_ARG), clamped to 768;
 * an unknown mode: DREPHIP_ERR_ARG.  A new context takes the mode from the
 * environment variable DREPHIP_RECT_BAND (auto | off | force) and the cap from
 * DREPHIP_RECT_BAND_CAP when they are set, read at creation. */
#define DREPHIP_RECT_BAND_AUTO  0  /* under DREPHIP_AP_AUTO: tables to s = 2048, the band kernel above (the default) */
#define DREPHIP_RECT_BAND_OFF   1  /* k_rect_merge above the tables, as before the band kernel */
#define DREPHIP_RECT_BAND_FORCE 2  /* the band kernel at every s (tests: small caps make many bands of small sketches) */
int drephip_set_rect_band(drephip_ctx *ctx, int mode, uint32_t band_cap /* 1..1024, clamped to 768 */);
/* The last rectangle call that ran (any drephip_dist_rect* form; an empty call
 * leaves it): *kernel = the kernel chosen for its counts (DREPHIP_AP_TABLE /
 * _BAND / _MERGE; 0 before the first call), *fallback = 1 when a band table
 * could not be built and the call's (or a row block's) rows were rerun by
 * k_rect_merge.  Either pointer may be NULL. */
int drephip_last_rect_info(drephip_ctx *ctx, int *kernel, int *fallback);
/* The rectangle's two-set shared-hash screen (every drephip_dist_rect* form in
 * front of the table and band kernels; k_rect_merge -- DREPHIP_AP_MERGE,
 * drephip_dist_rect_merge_device, DREPHIP_RECT_BAND_OFF above s = 2048 -- is
 * never screened).  Per block of query rows the block's valid query entries
 * are sorted by hash, the reference matrix is streamed once past them, and the
 * (row tile, reference) cells that hold an equal valid hash are marked; the
 * kernels run on the marked cells only (their RECT, LIST flavours) and every
 * other cell is common 0, denom min(s, nq + nr).  Exact: the outputs equal the
 * unscreened call's bit for bit.  Under AUTO a block is screened only when a
 * count pass over every reference finds checks * ratio <= rows * N * s (checks:
 * the marking's bit tests; ratio 16, DREPHIP_SCREEN_RATIO), else it runs every
 * item as without the screen.  A new context takes the mode from the
 * environment variable DREPHIP_RECT_SCREEN (auto | off | force), read at
 * creation.  DREPHIP_RECT_SCREEN_MIN_N / _MIN_Q (read per call) lower AUTO's
 * floors and DREPHIP_RECT_SCREEN_BLOCK_ROWS the rows per block, for tests.
 * With DREPHIP_DEBUG set, one line per screened block goes to stderr:
 * "[drephip] rect screen plan: R .. C .. tiles .. marked .. items .. slots ..
 * pieces .." (row tiles of the block, marked cells, LIST items, item slots
 * with the idle ones, kernel dispatches; nothing is dispatched at 0 slots);
 * an unscreened block prints the "rect plan:" / "rect band plan:" line. */
#define DREPHIP_RECT_SCREEN_AUTO  0  /* from 4096 references and 2048 query rows of a call on (the default) */
#define DREPHIP_RECT_SCREEN_OFF   1  /* every (row tile, column tile) item runs */
#define DREPHIP_RECT_SCREEN_FORCE 2  /* every call of any size, no verdict */
int drephip_set_rect_screen(drephip_ctx *ctx, int mode);
/* The screen of the last rectangle call (zeros when it did not run): *used = 1
 * when at least one block ran on its marked cells only; the blocks it looked
 * at; the query entries sorted and their distinct hashes (summed over blocks);
 * the count pass's checks (0 under FORCE, which skips it); the marked cells of
 * the screened blocks; the blocks the verdict sent to the unscreened plan.
 * Any pointer may be NULL.  drephip_last_rect_info keeps its meaning: the
 * kernel that computed the cells. */
int drephip_last_rect_screen_stats(drephip_ctx *ctx, int *used, uint32_t *blocks, uint64_t *query_entries,
                                   uint64_t *distinct, uint64_t *checks, uint64_t *marked, uint32_t *dense_blocks);
/* The screen's phases of the last rectangle call in milliseconds, summed over
 * blocks: sort (keys, radix sort, run heads), count pass, marking, lists, fill.
 * Measured only while bit 4 of drephip_set_timing is set (else zeros). */
int drephip_last_rect_screen_ms(drephip_ctx *ctx, double ms[5]);
/* DREPHIP_RECT_SCREEN's parser: "auto", "off" or "force" -> *mode (anything
 * else reads as auto, as at context creation).  Needs no device. */
int drephip_rect_screen_mode_of(const char *text, int *mode);
/* The same rectangle by k_rect_merge whatever s and whatever the band mode
 * (`mash dist <reference.msh> <query.msh>` by Mash's own loop): the
 * independent cross-check. */
int drephip_dist_rect_merge_device(drephip_ctx *ctx, const uint64_t *d_qhashes, const uint32_t *d_qnhash, uint32_t Q,
                                   const uint64_t *d_rhashes, const uint32_t *d_rnhash, uint32_t N, uint32_t q0,
                                   uint32_t q1, uint16_t *d_common, uint16_t *d_denom /* nullable */, void *stream);
/* The host form of `mash dist <reference.msh> <query.msh>`: both matrices are
 * staged on the context's device and checked first (every row ascending and
 * distinct, nhash <= s, UINT64_MAX past nhash; DREPHIP_ERR_ARG otherwise). */
int drephip_dist_rect(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash, uint32_t Q,
                      const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N, uint32_t q0, uint32_t q1,
                      uint16_t *common_out, uint16_t *denom_out /* nullable */);
/* `mash dist <reference.msh> <query.msh>` listing only the pairs that share a
 * hash: records of 4 uint32 {q, r, common, denom} (q the query row, r the
 * reference row), common > 0, each pair at most once, order unspecified.  The
 * cap / n_pairs contract is that of drephip_allpairs_sparse_device: cap = 0
 * only counts; with too few slots only [0, cap) is written, the call returns
 * DREPHIP_ERR_NOMEM and *n_pairs is the size needed.  s <= 2048: the RECT
 * kernel stages and appends the records itself, no rectangle is written.
 * Above, and for DREPHIP_AP_MERGE: query-row blocks of at most 2^28 pairs
 * (at least one row; DREPHIP_RECT_BLOCK_ROWS sets fewer rows, for tests),
 * each filled into a scratch rectangle of the context by the kernel
 * drephip_dist_rect_device picks (the RECT band kernel, with its rerun per
 * block, or k_rect_merge) and compacted.  With
 * DREPHIP_DEBUG set, the RECT kernel's plan is printed to stderr, one line
 * per call: "[drephip] rect plan: R .. C .. items .. slots .. gmax .. pieces
 * .." (row tile, column tile, (row tile, column tile) pairs, item slots with
 * the idle ones, largest group, kernel dispatches). */
int drephip_dist_rect_sparse_device(drephip_ctx *ctx, const uint64_t *d_qhashes, const uint32_t *d_qnhash, uint32_t Q,
                                    const uint64_t *d_rhashes, const uint32_t *d_rnhash, uint32_t N, uint32_t q0,
                                    uint32_t q1, uint32_t *d_pairs /* cap x 4 */, uint64_t cap, uint64_t *n_pairs,
                                    void *stream);
/* The host form of the record call (`mash dist <reference.msh> <query.msh>`,
 * non-zero pairs only); both matrices checked as drephip_dist_rect does. */
int drephip_dist_rect_sparse(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash, uint32_t Q,
                             const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N, uint32_t q0, uint32_t q1,
                             uint32_t *pairs /* cap x 4 */, uint64_t cap, uint64_t *n_pairs);
/* Best hits of `mash dist <reference.msh> <query.msh>`: for each query row q
 * of [q0, min(q1, Q)) the `top` (1..64, else DREPHIP_ERR_ARG) references
 * nearest to it by Mash distance among those that share a hash with it
 * (common > 0; the 0 / 0 pair of two empty sketches is never listed, as in the
 * record form).  Hit t of row q is 4 uint32 {r, common, denom, 0} at
 * ((q - q0) * top + t) * 4, common and denom exactly drephip_dist_rect's cell
 * (q, r); d_count[q - q0] = min(top, references with common > 0); the slots at
 * or past it hold {0xFFFFFFFF, 0, 0, 0}; nothing else is written.  Order:
 * larger common / denom first, compared as exact rationals (for common > 0
 * the Mash distance falls strictly with the ratio and never reaches its clamp
 * at 1, denom <= 32767), equal ratios by smaller r: a total order, so the
 * result is deterministic, and a query that is also a reference lists itself
 * first with common == denom.  Q == 0, N == 0 or q0 >= q1: DREPHIP_OK,
 * nothing written; null pointers: DREPHIP_ERR_ARG.  No Q x N buffer: the
 * query rows are walked in blocks of at most 2^28 cells (at least one row;
 * DREPHIP_RECT_TOP_BLOCK_ROWS sets fewer rows, for tests), each block's counts
 * by the rectangle's kernel (as drephip_dist_rect_device picks it: tables,
 * the RECT band kernel above s = 2048 with its rerun per block, or the merge;
 * DREPHIP_AP_BAND: DREPHIP_ERR_UNSUPPORTED) into a scratch rectangle of the
 * context (common + denom, at most 1 GB), then k_rect_top selects per row.
 * Blocking, on the caller's stream; a pending drephip_allpairs_device_async
 * is waited for first.  drephip_last_kernel_ms `which` 5 is the selection
 * kernel summed over the blocks, 2 / 3 the counts kernel and its table build. */
int drephip_dist_rect_top_device(drephip_ctx *ctx, const uint64_t *d_qhashes, const uint32_t *d_qnhash, uint32_t Q,
                                 const uint64_t *d_rhashes, const uint32_t *d_rnhash, uint32_t N, uint32_t q0,
                                 uint32_t q1, uint32_t top, uint32_t *d_hits /* (q1 - q0) x top x 4 */,
                                 uint32_t *d_count /* q1 - q0 */, void *stream);
/* The host form of the best hits; both matrices staged and checked as
 * drephip_dist_rect does. */
int drephip_dist_rect_top(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash, uint32_t Q,
                          const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N, uint32_t q0, uint32_t q1,
                          uint32_t top, uint32_t *hits /* (q1 - q0) x top x 4 */, uint32_t *count /* q1 - q0 */);

/* ---------------------------------------------------------------- significance
 * Replaces: the p-value column (the fourth) and the options -v <max p-value>
 * and -d <max distance> of `mash dist`, drep/d_cluster.py:569-573, for every
 * form of the call that lists records or hits.  Mash's definition, with the
 * context's k and s (not the pair's denominator):
 *   kspace = 4^k;  px = 1/(1 + kspace/len_a),  py = 1/(1 + kspace/len_b);
 *   r = px py / (px + py - px py);  M = kspace (px + py) / (1 + r);
 *   n = floor(min(M, s));
 *   p = 1 if common == 0, 0 if common > n, else P(X >= common), X ~ Binomial(n, r).
 * r and n are formed with these IEEE double operations in this order.  The
 * tail is summed with IEEE + - x / only (drep_amd/csrc/pvalue.h), by the same
 * inline functions on the host and in the kernels, compiled without FMA
 * contraction: the host and device forms agree bit for bit.  A value below
 * 2^-1022 is 0.0 (no subnormals); the relative error of the others is below
 * 1e-11 (about (n + 3 common) 2^-53).
 *
 * drephip_pvalue_eval.  Replaces: the p-value column of `mash dist`
 * (drep/d_cluster.py:569-573) for n (common, len_a, len_b) triples, on the
 * host: no context, no GPU.  r_out / n_out (nullable) receive r and n.  A
 * length of 0 with common > 0 cannot occur (a genome shorter than k has an
 * empty sketch): DREPHIP_ERR_ARG. */
int drephip_pvalue_eval(int k, uint32_t s, const uint32_t *common, const uint64_t *len_a, const uint64_t *len_b,
                        uint64_t n, double *pval, double *r_out /* nullable */, uint32_t *n_out /* nullable */);
/* drephip_pvalue_records_device.  Replaces: the p-value column of `mash dist`
 * (drep/d_cluster.py:569-573) for n records {a, b, common, denom} as the
 * sparse calls list them (kernel k_pvalue_records, one lane per record): a
 * indexes d_len_a (n_a entries), b indexes d_len_b (n_b entries) -- triangle
 * records pass one array twice, rectangle records {q, r} the query and the
 * reference lengths.  Writes exactly n doubles.  n == 0: DREPHIP_OK; null
 * pointers: DREPHIP_ERR_ARG.  The value of a record that names a genome
 * outside its array is NaN, that of one with a zero length and common > 0 is
 * unspecified.  Blocking, on the caller's stream. */
int drephip_pvalue_records_device(drephip_ctx *ctx, const uint32_t *d_records /* n x 4 */, uint64_t n,
                                  const uint64_t *d_len_a, uint32_t n_a, const uint64_t *d_len_b, uint32_t n_b,
                                  double *d_pval, void *stream);
/* drephip_pvalue_records.  Replaces: the same column, the host form: the
 * records and lengths are staged and checked first (a < n_a, b < n_b,
 * common <= denom <= s, a length >= 1 wherever common > 0; DREPHIP_ERR_ARG
 * otherwise). */
int drephip_pvalue_records(drephip_ctx *ctx, const uint32_t *records /* n x 4 */, uint64_t n, const uint64_t *len_a,
                           uint32_t n_a, const uint64_t *len_b, uint32_t n_b, double *pval);
/* drephip_pvalue_hits_device.  Replaces: the p-value column of `mash dist`
 * (drep/d_cluster.py:569-573) for the best hits of drephip_dist_rect_top*:
 * d_hits holds rows x top hits {r, common, denom, 0}, d_count the listed hits
 * per row, d_qlen the rows' query lengths (from q0 on), d_rlen the N reference
 * lengths.  d_pval (rows x top) receives the p-value of every listed hit and
 * 1.0 in the slots at or past the row's count.  Blocking, on the caller's
 * stream. */
int drephip_pvalue_hits_device(drephip_ctx *ctx, const uint32_t *d_hits, const uint32_t *d_count, uint32_t rows,
                               uint32_t top, const uint64_t *d_qlen, const uint64_t *d_rlen, uint32_t N,
                               double *d_pval /* rows x top */, void *stream);
/* drephip_records_filter_device.  Replaces: the options -v <max p-value> and
 * -d <max distance> of `mash dist` (drep/d_cluster.py:569-573) on a record
 * list: record t is kept when d_pval[t] <= max_p and common >= d_cmin[denom].
 * d_pval NULL: no p-value test; d_cmin NULL: no distance test.  d_cmin has
 * s + 1 entries, built by the caller from drephip_distance_lut: cmin[d] = the
 * smallest c with lut_d[c] <= max distance, d + 1 when there is none -- the
 * rule is then the float64 comparison itself.  Stable: the survivors keep
 * their order, in d_out (and their p-values in d_pval_out, nullable);
 * *n_out = their number.  The outputs hold up to n entries and must not alias
 * the inputs.  max_p outside [0, 1] or NaN: DREPHIP_ERR_ARG.  Lists of more
 * than 2^26 records are filtered in pieces (DREPHIP_FILTER_CHUNK sets fewer
 * records per piece, for tests).  Blocking, on the caller's stream. */
int drephip_records_filter_device(drephip_ctx *ctx, const uint32_t *d_records, const double *d_pval /* nullable */,
                                  uint64_t n, double max_p, const uint32_t *d_cmin /* nullable, s + 1 */,
                                  uint32_t *d_out, double *d_pval_out /* nullable */, uint64_t *n_out, void *stream);
/* drephip_allpairs_sparse_sig, drephip_dist_rect_sparse_sig.  Replace:
 * `mash dist -v <max_p> -d <max distance>` (drep/d_cluster.py:569-573) as
 * records: the host forms drephip_allpairs_sparse / drephip_dist_rect_sparse
 * with the genomes' lengths, max_p, a host cmin (nullable, as above), a p-value
 * per record (pval, nullable, cap entries) and *n_listed (nullable), the
 * records before the filter.  The matrices are staged and checked as in those
 * calls (and a genome with a non-empty sketch must have a length >= 1), the
 * device record call lists the pairs into context scratch (a counting run,
 * then room for exactly that many), the p-values and the filter run there, and
 * only the survivors are copied out, in the device call's order.  The cap /
 * n_pairs / DREPHIP_ERR_NOMEM contract is that of the record calls, applied to
 * the filtered list.  The record calls themselves are unchanged. */
int drephip_allpairs_sparse_sig(drephip_ctx *ctx, const uint64_t *hashes, const uint32_t *nhash, uint32_t N,
                                uint32_t row0, uint32_t row1, const uint64_t *length /* N */, double max_p,
                                const uint32_t *cmin /* nullable, s + 1 */, uint32_t *pairs /* cap x 4 */, uint64_t cap,
                                double *pval /* nullable, cap */, uint64_t *n_pairs, uint64_t *n_listed /* nullable */);
int drephip_dist_rect_sparse_sig(drephip_ctx *ctx, const uint64_t *qhashes, const uint32_t *qnhash, uint32_t Q,
                                 const uint64_t *rhashes, const uint32_t *rnhash, uint32_t N, uint32_t q0, uint32_t q1,
                                 const uint64_t *qlength /* Q */, const uint64_t *rlength /* N */, double max_p,
                                 const uint32_t *cmin /* nullable, s + 1 */, uint32_t *pairs /* cap x 4 */, uint64_t cap,
                                 double *pval /* nullable, cap */, uint64_t *n_pairs, uint64_t *n_listed /* nullable */);
/* drephip_write_mash_table_rect.  Replaces: the text of
 * `mash dist <reference.msh> <query.msh>` (the two-file form of
 * drep/d_cluster.py:569-573): Q x N lines, the query as the outer loop,
 * "rnames[r]\tqnames[q]\t%g dist\t%g p-value\tcommon/denom\n" of cell
 * q * N + r of the row-major rectangle (denom NULL = s for every cell), the
 * distances and p-values the caller's.  No diagonal rule: a query that is also
 * a reference prints its cell as computed.  Host only; rows formatted on
 * `threads` threads (0 = all), written in order. */
int drephip_write_mash_table_rect(const char *path, const char *const *rnames, uint32_t N, const char *const *qnames,
                                  uint32_t Q, const uint16_t *common, const uint16_t *denom /* nullable */, uint32_t s,
                                  const double *dist, const double *pval, int threads);

/* ---------------------------------------------------------- primary clustering
 * Replaces: scipy.cluster.hierarchy.linkage(squareform(dist), method) in
 * cluster_hierarchical (drep/d_cluster.py:447-453), called from
 * cluster_mash_database (598-630) -- the O(n^2) step of primary clustering.
 * Result: the (n-1) x 4 linkage matrix Z, bit-identical to scipy's (its
 * nn_chain for complete/average/weighted/ward, mst_single_linkage for single,
 * then its stable sort and relabel).  Method codes are scipy's.  Ward runs on
 * the dense path only (its update moves a pair at 1.0, so the components of
 * the pairs below 1.0 are not independent: no sparse form) and needs
 * distances >= 0: a negative entry of y, M or the distance table fails the
 * call with DREPHIP_ERR_UNSUPPORTED ("ward needs distances >= 0"; scipy
 * returns NaN rows there).  centroid (3) and median (4) are refused: scipy
 * runs them through another algorithm (fast_linkage). */
#define DREPHIP_LINK_SINGLE 0
#define DREPHIP_LINK_COMPLETE 1
#define DREPHIP_LINK_AVERAGE 2
#define DREPHIP_LINK_WARD 5          /* dense path only */
#define DREPHIP_LINK_WEIGHTED 6
/* Two paths, chosen per call (drephip_set_linkage_path):
 *  - sparse: when no distance exceeds 1.0 -- Mash's distance of two genomes
 *    sharing no hash is exactly 1.0, the top of its range -- scipy's algorithm
 *    is replayed on the host over the pairs below 1.0 only (one small dense
 *    matrix per connected component of those pairs; the counts path extracts
 *    them on the GPU).  Bit-identical to scipy.  Used automatically when the
 *    per-component matrices fit 2^28 f64 cells (DREPHIP_LINK_SPARSE_CELLS);
 *    when the path is forced (and in drephip_linkage_sparse) components too
 *    large for matrices run scipy's chain over sparse rows instead (no
 *    matrix; host time grows with the rows' lengths: ~1 s at 2x10^4 genomes
 *    with ~100 chance links each);
 *  - dense: the n x n f64 matrix in HBM, one GPU launch per chain step. */
#define DREPHIP_LINK_PATH_AUTO 0
#define DREPHIP_LINK_PATH_DENSE 1
#define DREPHIP_LINK_PATH_SPARSE 2   /* fails (DREPHIP_ERR_UNSUPPORTED) where no sparse form exists (ward: always) */
/* (a new context starts at DREPHIP_LINK_PATH_AUTO, or at the path named by the
 * environment variable DREPHIP_LINK_PATH = auto | dense | sparse) */
int drephip_set_linkage_path(drephip_ctx *ctx, int path);
/* From a host condensed distance vector y (n(n-1)/2 doubles, scipy order). */
int drephip_linkage(drephip_ctx *ctx, const double *y, uint32_t n, int method, double *Z /* (n-1)*4 */);
/* From the device-resident all-pairs output of drephip_allpairs_device (rows
 * 0..n-1 in one segment): distance of pair (i, j) = lut[lut_off[denom] +
 * common] (denom = s when d_denom is NULL; lut_off has s+1 entries, -1 for a
 * denominator that does not occur), placed at row/column perm[i], perm[j] of
 * the linkage input.  The counts are read after all work queued on `stream`
 * (and after a pending drephip_allpairs_device_async on this context).  A pair
 * whose denominator has no table, or whose count exceeds it, fails the call
 * (DREPHIP_ERR_ARG).  Blocking. */
int drephip_linkage_counts_device(drephip_ctx *ctx, const uint16_t *d_common, const uint16_t *d_denom,
                                  uint32_t n, const uint32_t *perm, const double *lut, uint32_t lut_len,
                                  const int32_t *lut_off, int method, double *Z /* (n-1)*4 */, void *stream);

/* From the host n x n float32 matrix the reference's pivot produces
 * (cluster_mash_database, drep/d_cluster.py:619-621: db.pivot(genome1,
 * genome2, dist) -> cluster_hierarchical's squareform -> linkage, 445-453):
 * Z = scipy.cluster.hierarchy.linkage(squareform(M), method).  The matrix is
 * copied to the device, where squareform's checks run (M == M^T element by
 * element, a zero diagonal) and linkage's (finite values), and the f64 linkage
 * input is built from the upper triangle, as squareform takes it.  A failed
 * check fails the call with DREPHIP_ERR_ARG and scipy's message ("Distance
 * matrix 'X' must be symmetric.", "Distance matrix 'X' diagonal must be
 * zero.", "The condensed distance matrix must contain only finite values.").  Dense path;
 * blocking. */
int drephip_linkage_square(drephip_ctx *ctx, const float *M, uint32_t n, int method, double *Z /* (n-1)*4 */);

/* ------------------------------------------------------------ Mdb on the host
 * The N^2-row Mdb table all_vs_all_MASH returns (drep/d_cluster.py:575-596),
 * filled from the condensed all-pairs result without the reference's text
 * round trip: row t = q N + r is (genome1 = genome r, genome2 = genome q) --
 * `mash dist` prints the query as the outer loop -- with
 *   dist[t] = 0 for r == q, else lut32[lut_off[denom] + common] of the pair
 *            (the float32 values the reference's read_csv parses from Mash's
 *            %g text, one table per denominator; denom NULL = s for every pair),
 *   sim[t]  = 1.0f - dist[t] (d_cluster.py:584, IEEE float32),
 *   g1[t] = codes[r], g2[t] = codes[q] (category codes, code_bytes 1, 2 or 4).
 * A pair whose denominator has no table, or whose count exceeds it, fails the
 * call (DREPHIP_ERR_ARG).  sim, g1, g2 nullable.  Host threads (0 = all). */
int drephip_mdb_square(uint32_t N, const uint16_t *common, const uint16_t *denom /* nullable */, uint32_t s,
                       const float *lut32, uint32_t lut_len, const int32_t *lut_off /* s+1 */,
                       const int32_t *codes /* N */, int code_bytes, void *g1, void *g2, float *dist,
                       float *sim, int threads);

/* The pivot of cluster_mash_database (d_cluster.py:620,
 * db.pivot(index="genome1", columns="genome2", values="dist")) on category
 * codes.  drephip_pivot_scan: which of the ncat categories occur in each
 * column (present1/present2), and *period = n when the rows have the layout
 * all_vs_all_MASH returns (codes1 repeating with period n, codes2 constant on
 * each block of n rows), else 0.  A negative code (a missing value) fails with
 * DREPHIP_ERR_UNSUPPORTED (the caller pivots with pandas).
 * drephip_pivot_fill: out[pos1[c1] * n2 + pos2[c2]] = vals of every row
 * (pos: the category's row/column of the pivot, -1 if absent); cells no row
 * names are NaN; two rows naming one cell fail with DREPHIP_ERR_ARG ("Index
 * contains duplicate entries, cannot reshape", pandas' error).  A period from
 * the scan (with n == n1 and nrows == n1 n2) takes the blocked transpose
 * instead of the scatter.  Host threads (0 = all). */
int drephip_pivot_scan(uint64_t nrows, const void *codes1, const void *codes2, int code_bytes, uint32_t ncat,
                       uint8_t *present1, uint8_t *present2, uint64_t *period, int threads);
int drephip_pivot_fill(uint64_t nrows, const void *codes1, const void *codes2, int code_bytes, const int32_t *pos1,
                       const int32_t *pos2, uint32_t ncat, const float *vals, uint32_t n1, uint32_t n2,
                       uint64_t period, float *out, int threads);

/* The sparse path on its own, no context or GPU: the npairs pairs (i[t], j[t])
 * with distance v[t] in [0, 1), each unordered pair at most once; every pair
 * not listed is at 1.0.  Z as scipy.cluster.hierarchy.linkage(squareform(D),
 * method) of that matrix.  DREPHIP_ERR_UNSUPPORTED when the per-component
 * matrices exceed 2^31 cells. */
int drephip_linkage_sparse(uint32_t n, uint64_t npairs, const uint32_t *i, const uint32_t *j, const double *v,
                           int method, double *Z /* (n-1)*4 */);

/* Which path the last drephip_linkage* call on this context took (sparse = 1)
 * and its pair list: pairs below 1.0, components with >= 2 members and the
 * largest one's size (0 for single linkage). */
int drephip_last_linkage_info(drephip_ctx *ctx, int *sparse, uint64_t *pairs, uint32_t *components,
                              uint32_t *largest);

/* Allocates (grow-only, kept in the context) the n x n f64 device matrix the
 * next linkage call of size <= n uses, so that a caller can pay the
 * allocation (80 GB at n = 10^5) outside the clustering step, e.g. before the
 * sketch/all-pairs stages.  Same limits as drephip_linkage. */
int drephip_linkage_reserve(drephip_ctx *ctx, uint32_t n);

/* Step launches of the last linkage call's nearest-neighbour chain that did
 * work (complete / average / weighted on the dense GPU path: ~1.2-1.35 per
 * merge); 0 after the sparse path and for single linkage (Prim). */
int drephip_last_linkage_launches(drephip_ctx *ctx, uint64_t *launches);

/* Host wall-clock split of the last drephip_linkage* call on this context
 * (seconds): the matrix allocation (0 when reserved/reused), the matrix build,
 * the chain (or MST) steps including their setup, the Z readback + scipy's
 * stable sort and relabel, and the whole call. */
int drephip_last_linkage_stats(drephip_ctx *ctx, double *alloc_s, double *matrix_s, double *chain_s,
                               double *finish_s, double *wall_s);

/* HIP-event timing of kernel launches: `kernels` is a bitmask of the kernels
 * to bracket with events (bit w = `which` w of drephip_last_kernel_ms; -1 =
 * all, 0 = none).  Each event pair adds a few microseconds of idle time
 * between dispatches, so a benchmark times only the kernel it reports. */
int drephip_set_timing(drephip_ctx *ctx, int kernels);

/* Per-launch timing of the last sketch/allpairs call on this context
 * (milliseconds, from HIP events on the launch stream): which = 0 sketch hash
 * kernel, 1 sketch finalize kernel, 2 allpairs kernel, 3 table build kernel,
 * 4 the shared-hash screen (grouping + lists, including its host round trips),
 * 5 the best-hits selection kernel (drephip_dist_rect_top*).
 * Returns the count of launches summed into *ms. */
int drephip_last_kernel_ms(drephip_ctx *ctx, int which, double *ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif /* DREPHIP_H */
