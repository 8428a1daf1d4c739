/* clair_host.h -- C ABI of the host-side helpers around the MI355X forward pass (libclair_host.so, plain C++, no HIP).
 *
 * These are the SURVEY.md section 8(f) "next" rows: the callers either side of the hot path that cap end-to-end
 * throughput once the network runs at millions of candidates per second.  Every function restates a piece of the
 * reference's Python (file:line below) and is pinned, byte for byte, against the build's Python counterpart in
 * clair_amd/ (which is itself pinned against fixtures minted from the real reference, tests/golden/).
 *
 * Convention: functions return 0 on success, non-zero on failure with a message in clair_host_last_error()
 * (thread-local).  Plain pointers and sizes only. */
#ifndef CLAIR_HOST_H
#define CLAIR_HOST_H
#include <stdint.h>
#include "clair_call.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CLAIR_HOST_ABI_VERSION 6
#define CLAIR_HOST_VALUES 1056      /* 33 positions x 8 rows x 4 channels (shared/param.py:9-13) */

int clair_host_abi_version(void);
const char *clair_host_last_error(void);
/* worker threads a call over `work_items` lines / candidates uses: CLAIR_HOST_THREADS from the environment, else up to 16
 * hardware threads, one per 128 items (results do not depend on it: rows keep their input order) */
int clair_host_threads(int work_items);
/* CRC32C (Castagnoli) of a byte range -- the checksum of TensorFlow's bundle format (clair_amd/tf_bundle.py); "123456789" -> 0xE3069283 */
uint32_t clair_host_crc32c(const uint8_t *data, int64_t n);

/* raw pileup counts -> network input (clair/utils.py:96-98: X[:,:,:,1:] -= X[:,:,:,0:1] after the float32 conversion of :81-83):
 * n_quads groups of four channels (33 x 8 per candidate); x[4q] = c[4q], x[4q+k] = c[4q+k] - c[4q].  int16 and int32 counts. */
int clair_host_counts_to_input_i16(const int16_t *counts, int64_t n_quads, float *x);
int clair_host_counts_to_input_i32(const int32_t *counts, int64_t n_quads, float *x);

/* -- ingest: the parsing work of clair/utils.py:72-109 (tensor_generator_from) for one chunk of text ---------------
 * Record format (dataPrepScripts/CreateTensor.py:60-65): "ctg pos refseq33 v0 ... v1055", whitespace separated.
 * buf[0..len) is consumed line by line ('\n'; a last line without '\n' counts only when `final` is non-zero) until
 * max_rows lines have been TAKEN (utils.py:79 counts dropped rows too) or the complete lines run out.  Per line:
 *   - the last 1056 columns -> float32 (utils.py:81-83); exactly three columns must precede them (utils.py:86);
 *   - rows whose centre base refseq[16] is not an IUPAC code are dropped (utils.py:90-91, shared/utils.py:24-27);
 *   - kept row k: x[k*1056 ..] = values with channels 1..3 -= channel 0 (utils.py:96-98);
 *     tok[k*6 ..] = (offset, length) pairs of ctg, pos, refseq inside buf.
 * Outputs: *rows_taken, *rows_kept, *bytes_consumed (start of the first line not taken).
 * Errors (malformed line: too few columns, not three leading columns, refseq shorter than 17, unparsable value) name
 * the 0-based line index inside this chunk; the reference raises a Python exception at the same places. */
int clair_host_parse_tensors(const char *buf, int64_t len, int final, int max_rows,
                             float *x, int32_t *tok, int *rows_taken, int *rows_kept, int64_t *bytes_consumed);

/* -- decode: probabilities -> VCF rows, the work of clair/call_var.py:589-1236 (possible_outcome_probabilites_from, output_from,
 *    output_with, batch_output) for one batch, in the configuration the GPU pipeline runs in: no BAM look-ups available (every
 *    look-up answers "", the reference's own fall-back to tensor-inferred bases, :520-524, :562-564), no --debug, no
 *    --output_for_ensemble.  x [n][1056] (channels 1..3 already minus channel 0), the four softmax arrays [n][21|3|33|33];
 *    meta + meta_tok: per candidate the (offset, length) pairs of ctg, pos, refseq inside meta (the layout
 *    clair_host_parse_tensors produces).  show_reference / haploid_* = the CLI flags (:1402-1429); qual_threshold < 0 = no
 *    --qual (FILTER "."); arith_numpy2 selects how QUAL and AF are rounded (clair_amd/call_var.py "Arithmetic mode").
 *    Rows are appended to out, each terminated by '\n', in input order; candidates that produce no row are skipped exactly as
 *    the reference skips them.  Byte-identical to clair_amd.call_var.VariantDecoder (tests/test_host.py). */
int clair_host_decode_rows(const float *x, const float *gt21, const float *genotype, const float *len1, const float *len2,
                           const char *meta, const int32_t *meta_tok, int n, int show_reference, int haploid_precision,
                           int haploid_sensitive, int qual_threshold, int arith_numpy2, char *out, int64_t out_cap,
                           int64_t *out_len, int *n_rows);
/* The same with a per-candidate status byte (status[n], may be NULL): bit 0 = the candidate produced a row, bit 1 = its
 * resolution passed a point where the reference consults the BAM when it has one (an indel of 16 bases or more,
 * call_var.py:498-524, 540-565; the second allele of an Ins/Ins call, :805-823).  A caller that holds a BAM decodes exactly the
 * candidates with bit 1 on its own look-up path and splices their rows in (clair_amd/call_var.py: VariantDecoder.decode_batch);
 * for every other candidate the BAM cannot change the row. */
int clair_host_decode_rows_ex(const float *x, const float *gt21, const float *genotype, const float *len1, const float *len2,
                              const char *meta, const int32_t *meta_tok, int n, int show_reference, int haploid_precision,
                              int haploid_sensitive, int qual_threshold, int arith_numpy2, char *out, int64_t out_cap,
                              int64_t *out_len, int *n_rows, uint8_t *status);

/* The two halves of that decode, apart (include/clair_call.h describes the 32-byte record between them).
 * clair_host_resolve_calls: everything arithmetic -- the ten outcome families, the iterative arg-max, genotype, depth, supporting
 *   reads, the probability QUAL starts from, the tensor's vote on inserted bases -- for n candidates; centre[2i] = the reference
 *   window's centre character refseq[16], centre[2i + 1] = min(length of refseq, 255).  It is the CPU twin of the GPU decode kernel
 *   (include/clair_amd.h: clair_submit_ex) and the yardstick that kernel is compared with bit for bit.
 * clair_host_format_calls: records + the candidates' text -> rows, exactly the rows clair_host_decode_rows_ex writes for the same
 *   candidates (that function IS resolve + format per candidate); status as there.
 * clair_host_centre_bytes: the centre[] array of a batch from its meta table. */
int clair_host_resolve_calls(const float *x, const float *gt21, const float *genotype, const float *len1, const float *len2,
                             const uint8_t *centre, int n, clair_call_t *calls);
int clair_host_format_calls(const clair_call_t *calls, const char *meta, const int32_t *meta_tok, int n, int show_reference,
                            int haploid_precision, int haploid_sensitive, int qual_threshold, int arith_numpy2, char *out,
                            int64_t out_cap, int64_t *out_len, int *n_rows, uint8_t *status);
int clair_host_centre_bytes(const char *meta, const int32_t *meta_tok, int n, uint8_t *centre);
/* clair_host_format_calls from the columns of binary tensor records (clair_amd/tensor_binary.py): contig names [n][37] with their
 * lengths, positions, reference windows [n][33] with their lengths -- no text table is built for the batch.  Same rows. */
int clair_host_format_calls_records(const clair_call_t *calls, const char *ctg, const uint8_t *ctg_len, const int64_t *pos, const char *seq,
                                    const uint8_t *seq_len, int n, int show_reference, int haploid_precision, int haploid_sensitive,
                                    int qual_threshold, int arith_numpy2, char *out, int64_t out_cap, int64_t *out_len, int *n_rows,
                                    uint8_t *status);

/* -- pileup: alignments -> [33][8][4] count windows, the work of dataPrepScripts/CreateTensor.py:179-394 (OutputAlnTensor) and
 *    :29-65 (generate_tensor) as a streaming builder.  The caller supplies what the reference obtains from its sub-processes:
 *    the reference slice `samtools faidx` printed (upper-cased, :137; reference_start_0_based = 0 or region start - 1, :217), the
 *    candidate positions (column 2 of the candidate rows, 1-based, those outside [ctgStart, ctgEnd] already dropped, :86-92, in
 *    stream order) and the text `samtools view` prints.  The builder replays the reference's rules: candidates become known
 *    100 000 bp ahead of the reads (:274-275); mapping-quality filter (:268-269); at most dcov reads per start position
 *    (:277-284); windows open / close as the CIGAR walk passes centre-17 / centre+17 (:286-371; consider_left_edge: at any
 *    walked position inside, :95-100); a window is finished when a read with a new start position begins beyond it (:373-386)
 *    or at clair_host_pileup_finish (:388-394), in first-touch order, and dropped when its centre depth is below min_coverage or
 *    it would start before the loaded reference (:58-59); available_slots is the reference's budget of outstanding
 *    (window, base) tuples (5 000 000, :181): bases are dropped once it is used up, exactly where the reference drops them
 *    (within one reference position the windows are served in the order clair_host_pileup_set_order selects).  force_general_path != 0 selects the hash-map twin of the sorted-candidates fast path (tests).
 *    Pinned byte for byte against records minted from the real script (tests/golden/pileup_ct_*.json.gz). */
typedef struct clair_pileup clair_pileup_t;
int clair_host_pileup_create(const char *ref_seq, int64_t ref_len, int64_t reference_start_0_based, const int64_t *candidates,
                             int64_t n_candidates, int consider_left_edge, int dcov, int min_coverage, int min_mq,
                             int64_t available_slots, int force_general_path, clair_pileup_t **out);
void clair_host_pileup_destroy(clair_pileup_t *p);
/* The order in which a read base is offered to the windows open over it (CreateTensor.py:296-310), before the first alignment is fed.  It shows
 * in the records only where the budget of outstanding tuples runs out in the MIDDLE of one base.  0 (default): the order the windows were opened
 * in -- what an insertion-ordered set gives, i.e. the script under PyPy, the interpreter clair/callVarBam.py runs it with by default (--pypy);
 * 1: the iteration order of CPython's hash set, restated in host_pileup.cpp and pinned against records minted from the real script under
 * CPython with the budget binding (tests/golden/pileup_ct_budget_binds.json.gz). */
int clair_host_pileup_set_order(clair_pileup_t *p, int cpython_set);
/* test hook for that restatement: replay set operations (key >= 0: add(key); -(key + 1): remove(key)) -> the keys in iteration order */
int clair_host_pyset_order(const int64_t *ops, int64_t n_ops, int64_t *keys, int64_t capacity, int64_t *n_keys);
/* Consume SAM text line by line ('\n'; a last line without '\n' only when `final`): header lines ('@') are skipped, columns
 * FLAG, POS, MAPQ, CIGAR, SEQ are used (:252-263).  *bytes_consumed = start of the first line not consumed.  Errors (too few
 * columns, non-integer column, CIGAR longer than SEQ, position outside the loaded reference) name the 0-based line index since
 * creation; the reference raises a Python exception at the same places. */
int clair_host_pileup_feed(clair_pileup_t *p, const char *sam, int64_t len, int final, int64_t *bytes_consumed);
int clair_host_pileup_finish(clair_pileup_t *p);
int64_t clair_host_pileup_pending(const clair_pileup_t *p);   /* finished windows waiting to be taken */
/* Take up to max_rows finished windows: centres[k] (1-based), refseq[k*34 ..] (NUL-padded; 33 bases unless the loaded reference
 * ends inside the window, as the reference's slice :63), counts[k*1056 ..] = [33][8][4] int32. */
int clair_host_pileup_take(clair_pileup_t *p, int64_t max_rows, int64_t *centres, char *refseq, int32_t *counts, int64_t *n_taken);
/* Take finished windows as the reference's text records "ctg centre refseq v0 ... v1055\n" (:60-65), as many as fit in cap. */
int clair_host_pileup_take_text(clair_pileup_t *p, const char *ctg_name, char *out, int64_t cap, int64_t *out_len, int64_t *n_taken);
/* stats[0..3] = reads walked, windows open, slots left, 1 if the sorted-candidates path is in use */
int clair_host_pileup_stats(const clair_pileup_t *p, int64_t *stats);

/* -- candidates: alignments -> candidate sites, the work of dataPrepScripts/ExtractVariantCandidates.py:160-393 (make_candidates)
 *    in inference mode, streaming.  Per alignment of contig ctg_name (:279-281): mapping quality >= min_mq (:291), CIGAR not "*"
 *    and at least 55 % aligned (:143-157, 293); M/=/X bases are tallied per reference position under their IUPAC_base_to_ACGT base
 *    (N kept), an insertion / deletion counts once at the position before it (:298-316).  Positions before the current read's
 *    start are complete (:319): a position is a candidate when it lies in [ctg_start, ctg_end] (1-based; -1, -1 = no range) and in
 *    the bed intervals (0-based half-open, start == end widened by one, shared/interval_tree.py:30-32; n_bed = -1: no bed file),
 *    its reference base is an IUPAC code, depth = bases - I - D >= min_coverage, and either the most frequent tally is not the
 *    reference base or the second one reaches `threshold` of the depth (:357-371; ties keep the order A C G T I D N).
 *    Rows: "ctg pos refbase depth X n X n ... (7 pairs, descending)" (:379-383).  The training-set switches (--gen4Training,
 *    --var_fn, --outputProb) sample with Python's random module and are not restated. */
typedef struct clair_evc clair_evc_t;
int clair_host_evc_create(const char *ctg_name, const char *ref_seq, int64_t ref_len, int64_t reference_start_0_based,
                          int64_t ctg_start, int64_t ctg_end, const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed,
                          double min_coverage, double threshold, int min_mq, clair_evc_t **out);
void clair_host_evc_destroy(clair_evc_t *e);
int clair_host_evc_feed(clair_evc_t *e, const char *sam, int64_t len, int final, int64_t *bytes_consumed);
int clair_host_evc_finish(clair_evc_t *e);
int64_t clair_host_evc_pending(const clair_evc_t *e);
int64_t clair_host_evc_reads(const clair_evc_t *e);      /* alignments that passed the filters (:295) */
int clair_host_evc_take(clair_evc_t *e, int64_t max_rows, int64_t *positions, int64_t *n_taken);   /* 1-based positions only */
int clair_host_evc_take_text(clair_evc_t *e, char *out, int64_t cap, int64_t *out_len, int64_t *n_taken);

/* -- packed alignments for the device front end (include/clair_reads.h; include/clair_amd.h: clair_frontend_*).  One pass over
 *    `samtools view` text replaces the line handling of BOTH reference stages (ExtractVariantCandidates.py:266-295 and
 *    CreateTensor.py:251-287): an alignment is kept when either stage would walk it and carries one flag bit per stage --
 *    the candidate search wants RNAME == ctg_name, MAPQ >= evc_min_mq, CIGAR != "*" and >= 55 % aligned; the pileup wants
 *    MAPQ >= pile_min_mq, at most dcov alignments per start position (:277-287) and, when pile_start/pile_end (1-based inclusive,
 *    -1 -1 = none) are given, an overlap with that range as `samtools view ctg:start-end` computes it (the reference gives the two
 *    stages different regions, callVarBam.py:124-199).  Errors as clair_host_pileup_feed.  The slab grows until it is taken:
 *    ..._slab lends the arrays (valid until the next feed / reset), ..._reset starts the next slab; the dcov and sortedness state
 *    runs on across slabs.  stats[0..7] = alignments, operations, elements, SEQ bytes in the slab; CLAIR_FE_* bits seen so far;
 *    lines, candidate-search alignments, pileup alignments since creation. */
typedef struct clair_sampack clair_sampack_t;
struct clair_read;
struct clair_op;
int clair_host_sampack_create(const char *ctg_name, int dcov, int evc_min_mq, int pile_min_mq, int64_t pile_start, int64_t pile_end,
                              clair_sampack_t **out);
void clair_host_sampack_destroy(clair_sampack_t *p);
int clair_host_sampack_feed(clair_sampack_t *p, const char *sam, int64_t len, int final, int64_t *bytes_consumed);
int clair_host_sampack_stats(const clair_sampack_t *p, int64_t *stats);
int clair_host_sampack_slab(const clair_sampack_t *p, const struct clair_read **reads, const struct clair_op **ops, const uint32_t **op_elem,
                            const uint8_t **seq);
int clair_host_sampack_reset(clair_sampack_t *p);
/* keep != 0: pack for the indel look-up (include/clair_reads.h, "the indel look-up") -- every alignment of the contig with a CIGAR gets
 * CLAIR_READ_LOOKUP and stays in the slab even when neither stage walks it (low MQ, beyond --dcov: pysam's pileup applies neither,
 * clair/call_var.py:102-170).  Before the first feed.  Off (the default): slabs as ever, byte for byte. */
int clair_host_sampack_set_lookup(clair_sampack_t *p, int keep);
/* The indel look-up on the host (hostsrc/host_indel.cpp; the work of clair/call_var.py:102-170 for n positions at once): the twin of
 * clair_frontend_indel_table (include/clair_amd.h), same bytes, and what that function falls back to.  n_slabs slabs in feed order
 * (reads[s], n_reads[s], ops[s], n_ops[s], seq[s], seq_bytes[s]); positions[n] 1-based, strictly ascending; entries [n][capacity],
 * n_entries[n], depth[n], status[n] (CLAIR_LOOKUP_ENTRIES only).  Rows of `entries` beyond n_entries are zeroed. */
struct clair_indel_entry;
int clair_host_indel_table(const struct clair_read *const *reads, const int64_t *n_reads, const struct clair_op *const *ops, const int64_t *n_ops,
                           const uint8_t *const *seq, const int64_t *seq_bytes, int64_t n_slabs, const int64_t *positions, int64_t n,
                           struct clair_indel_entry *entries, int capacity, int32_t *n_entries, int32_t *depth, uint32_t *status);
/* CreateTensor.py's count of free tuple slots (:181, 283-289, 369-373) replayed from what the device counted: alignments in stream
 * order with the tuples each appended, candidate centres ascending with the tuples their windows held when released.  state[0] =
 * free slots (start: 5 000 000), state[1] = first centre not released yet (start: 0); carried from slab to slab.  *binds = 1 when
 * the count would have reached zero: the reference then drops bases in offer order and only the sequential code reproduces it. */
int clair_host_tuple_budget_binds(const struct clair_read *reads, const uint64_t *tuples, int64_t n_reads, const int64_t *centres,
                                  const uint64_t *window_tuples, int64_t n_centres, int64_t *state, int *binds);

/* -- BAM input without samtools (callVarBam --bam_reader native; hostsrc/host_bam.cpp, zlib).  What `samtools view -F 2316 <bam>
 *    <region>` does before it formats text: BGZF blocks inflated on `threads` threads (1 .. 16) with each block's CRC32 and ISIZE
 *    checked (errors name the block's compressed offset), the header's reference names and lengths, the region's chunks from a .bai
 *    (htslib's hts_itr_query) or a scan from the first record, and the walk over whole records that ends at the first record of the
 *    contig starting past the region (hts_itr_next).  A file that is not BGZF (SAM text, CRAM, plain gzip) is an error that says to
 *    use samtools.
 *    info[0..3] = references in the header, 1 if the BGZF EOF block is present, records handed out by this query, 1 if it used an index.
 *    query: beg1 / end1 1-based inclusive, -1 -1 = the whole contig; index_path NULL = scan.
 *    next: whole records (block_size field included) into buf[0..cap), at most max_records; offsets[k] = where record k starts;
 *    *n_records = 0 at the end.  The records are all those the index (or the scan) yields -- the view filter is the consumer's:
 *    clair_frontend_add_bam on the device, clair_host_bam_render here.
 *    voffset: BGZF virtual offset of record k of the last chunk next handed out (for messages).
 *    render: of n records, those `samtools view -F 2316` keeps for contig tid and the region, as the 11 mandatory SAM columns it prints
 *    (QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL; '*' for no CIGAR, no SEQ, QUAL 0xff; the CG:B:I CIGAR for the
 *    kSmN placeholder); *text is the handle's and valid until the next render.
 *    faidx: the bases of ctg:beg1-end1 (clamped; -1 -1 = whole contig) as `samtools faidx` prints them, case kept, line ends
 *    dropped; out NULL = *len only.
 *    set_inflater: from here on the BGZF blocks of a query are inflated by fn, batch_blocks (1 .. 16384) at a time, instead of by zlib
 *    on the thread pool (fn NULL: back to zlib).  fn gets n whole blocks (header and footer included) at cdata[in_at[i] .. + csize[i]),
 *    writes block i's out_len[i] (its ISIZE) bytes to out[out_at[i] ..] and sets status[i]: 0 ok, 1 corrupt deflate data, 2 inflated size
 *    differs from ISIZE, 3 CRC32 mismatch; it returns non-zero when it could not run.  The first non-zero status becomes the message the
 *    zlib path gives for that block, with its compressed offset.  libclair_amd's clair_inflate_blocks_cb is such a function (include/clair_amd.h,
 *    its handle as ctx): this library does not link HIP.  The header blocks read at open are inflated by zlib. */
typedef struct clair_bam clair_bam_t;
typedef int (*clair_host_inflate_fn)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                                     const int64_t *out_at, const int32_t *out_len, uint8_t *out, int32_t *status);
int clair_host_bam_open(const char *path, int threads, clair_bam_t **out);
void clair_host_bam_close(clair_bam_t *b);
int clair_host_bam_info(const clair_bam_t *b, int64_t *info);
int clair_host_bam_ref(const clair_bam_t *b, int tid, const char **name, int64_t *length);
int clair_host_bam_tid(const clair_bam_t *b, const char *name);
int clair_host_bam_query(clair_bam_t *b, const char *index_path, int tid, int64_t beg1, int64_t end1);
int clair_host_bam_next(clair_bam_t *b, uint8_t *buf, int64_t cap, int64_t *offsets, int64_t max_records, int64_t *len, int64_t *n_records);
int clair_host_bam_voffset(const clair_bam_t *b, int64_t k, uint64_t *voffset);
int clair_host_bam_render(clair_bam_t *b, const uint8_t *records, const int64_t *offsets, int64_t n, int tid, int64_t beg1, int64_t end1,
                          const char **text, int64_t *len);
int clair_host_faidx(const char *fasta, const char *ctg, int64_t beg1, int64_t end1, char *out, int64_t cap, int64_t *len);
int clair_host_bam_set_inflater(clair_bam_t *b, clair_host_inflate_fn fn, void *ctx, int batch_blocks);
/*    set_subsample: from here on render also drops what `samtools view -s` would (csrc/subsample_core.h, docs/subsample.md: the hash of the
 *    read name, XORed with the 32-bit word `seed` (0 .. 2^32 - 1) and mixed, at or above `frac`); frac <= 0 turns the rule off, frac >= 1
 *    keeps every record.  The twin of clair_frontend_bam_subsample (include/clair_amd.h); next frames records and is unchanged.
 *    subsample_keeps: the rule for one name -- name[0 .. n), or up to an earlier NUL -- -> 1 kept, 0 dropped, -1 for bad arguments. */
int clair_host_bam_set_subsample(clair_bam_t *b, int64_t seed, double frac);
int clair_host_subsample_keeps(const uint8_t *name, int64_t n, int64_t seed, double frac);

/* -- the host twin of the device inflate (hostsrc/host_inflate.cpp): the RFC 1951 decoder of csrc/inflate_core.h, the code the GPU runs,
 *    compiled for the host with its own CRC-32 (no zlib), so that it can be tested, fuzzed and run under the host sanitizer.  It accepts
 *    exactly the streams zlib's inflate(Z_FINISH) with windowBits = -15 accepts.
 *    _block: one raw deflate stream in[0 .. n_in) into out[0 .. cap); *status = 0 and *n_out, *crc32 (of the output) set when the final
 *    block ended within cap bytes, *status = 1 otherwise (*n_out = 0).  Input after the final block is ignored.
 *    _bgzf: one whole BGZF block (18-byte header, stream, CRC32, ISIZE <= 65536) as the device kernel treats it: out has room for
 *    ISIZE + 1 bytes; *status as clair_host_bam_set_inflater's.
 *    Both return non-zero only for bad arguments. */
int clair_host_inflate_block(const uint8_t *in, int64_t n_in, uint8_t *out, int64_t cap, int64_t *n_out, uint32_t *crc32, int *status);
int clair_host_inflate_bgzf(const uint8_t *block, int64_t csize, uint8_t *out, int64_t *n_out, int *status);

/* -- the host twin of the device deflate (hostsrc/host_deflate.cpp): the compressor of csrc/deflate_core.h, the code the GPU runs inside
 *    clair_deflate_blocks (include/clair_amd.h), compiled for the host (no zlib).  in[0 .. n_in), n_in <= 65280 (bgzip's block payload) ->
 *    one whole BGZF block in out[0 .. *n_out): 18-byte header with BSIZE, a raw deflate stream (dynamic Huffman blocks, or one stored block
 *    when that is not smaller), CRC-32, ISIZE.  out has room for 65536 bytes; the bytes beyond *n_out are zero.  The same input gives the
 *    same bytes here and on the device.  Returns non-zero only for bad arguments.  Re-entrant. */
int clair_host_deflate_bgzf(const uint8_t *in, int64_t n_in, uint8_t *out, int64_t *n_out);

/* -- the host twin of the device ensemble averaging (hostsrc/host_ensemble.cpp): csrc/ensemble_core.h, the code the GPU runs after each of
 *    the K forward passes of clair_submit_ensemble (include/clair_amd.h), compiled for the host.  It restates the reference's text chain
 *    value for value: '{:0.6f}' of every float32 probability (clair/call_var.py:950-1000), float() of those digits, the sum in input order
 *    and the division in double, '{:.6f}' of the mean (clair/post_processing/ensemble.py:33-43, :67), float32 of those digits
 *    (clair/call_var.py:1291).  docs/ensemble.md has the rule and why rint(mean * 1e6) is not it.
 *    _average: probs [models][count] float32, model order = summation order, 1 <= models <= 8 -> out [count].  models = 1 is not the
 *    identity: it rounds to six decimals, as the chain with one model does.
 *    _quantise: the integer of millionths '{:0.6f}' prints for each float32 (ties to even).  _value: float32 of "m / 10^6" for 0 <= m <= 10^6.
 *    NaN is out of scope. */
int clair_host_ensemble_average(const float *probs, int models, int64_t count, float *out);
int clair_host_ensemble_quantise(const float *p, int64_t count, int32_t *millionths);
int clair_host_ensemble_value(const int32_t *millionths, int64_t count, float *out);

/* -- the host twin of the device site table (hostsrc/host_sites.cpp): ensemble calling across BAMs, clair_sites_* of include/clair_amd.h in
 *    plain C++ over the same csrc/ensemble_core.h.  A table keyed by position: per site the number of runs that produced it, the sum of
 *    their re-read probabilities in run order (double), and window, centre bytes and seq of the first run that had it; sites are rows in
 *    first-seen order.  _begin_source: all positions of the next source, strictly ascending (*n_new: how many the table did not have).
 *    _add_rows: one run's packed rows probs [n][90] for candidates [first, first + n) of the current source; x [n][1056] float32,
 *    centre [n][2], seq [n][33] optional, taken by sites nobody wrote before.  _finish: the output list -- sites with at least min_count
 *    rows (clair/post_processing/ensemble.py:58-59), order 0 = first-seen (what the text filter prints), 1 = by position; may be repeated.
 *    _info / _rows / _windows: entries [first, first + n) of that list; _rows gives clair_ens_finish(sum, count) as float32 [n][90].
 *    Errors: positions not strictly ascending, a row range outside the current source or the output list, rows after _finish, a 65th row
 *    of a site. */
typedef struct clair_host_sites clair_host_sites_t;
int clair_host_sites_create(clair_host_sites_t **out);
void clair_host_sites_destroy(clair_host_sites_t *t);
int clair_host_sites_begin_source(clair_host_sites_t *t, const int64_t *positions, int64_t n, int64_t *n_new);
int clair_host_sites_add_rows(clair_host_sites_t *t, int64_t first, const float *probs, int64_t n, const float *x, const uint8_t *centre, const uint8_t *seq);
int clair_host_sites_finish(clair_host_sites_t *t, int min_count, int order, int64_t *n_out);
int clair_host_sites_info(clair_host_sites_t *t, int64_t first, int64_t n, int64_t *positions, int32_t *counts, uint8_t *seq);
int clair_host_sites_rows(clair_host_sites_t *t, int64_t first, int64_t n, float *out);
int clair_host_sites_windows(clair_host_sites_t *t, int64_t first, int64_t n, float *x);

/* -- the host twin of the device overlap filter (hostsrc/host_overlap.cpp): the walk of clair/post_processing/overlap_variant.py:237-267
 *    over rows reduced to spans, with the pair rule of csrc/overlap_core.h (which also lays the 24-byte span record out), the code the
 *    GPU runs inside clair_overlap_keep (include/clair_amd.h).  spans [n] in input order -> keep [n]: 1 for the rows the filter prints,
 *    0 for those it drops.  The text on either side is clair_amd/overlap_variant.py's; docs/overlap_variant.md has the rule. */
#ifndef CLAIR_OVERLAP_SPAN_T
#define CLAIR_OVERLAP_SPAN_T
typedef struct clair_overlap_span clair_overlap_span_t;
#endif
int clair_host_overlap_keep(const clair_overlap_span_t *spans, int64_t n, uint8_t *keep);

/* -- the host twin of the device training-set builder (hostsrc/host_train_set.cpp; docs/train_set.md), with the rules of
 *    csrc/train_set_core.h, the code the GPU runs inside clair_frontend_sample_candidates / clair_frontend_pair (include/clair_amd.h).
 *    Positions are 1-based; truth [n_truth] ascending (duplicates allowed); bed intervals of the contig sorted, merged, 0-based half-open,
 *    n_bed < 0 = no bed file.  _key: the key of a contig's draws, stage 1 = site sampling, 2 = pairing.  _sample: per position its class
 *    (0 outside, 1 near, 2 truth), its 53-bit draw and whether it is sampled (any of the three may be NULL), and the two counters of the
 *    sampled sites.  _pair_count: v = windows at a truth position, c = usable non-variant windows; _ratio: r = min(1, v amp / c), 1 for
 *    c == 0; _pair_keep: indices of the kept windows, the variant ones first, each part in input order.  _labels: the four true indices
 *    and the data-set flag per window (truth_labels [n_truth][4]; the last row of a position wins). */
int clair_host_train_set_key(const char *ctg_name, int64_t seed, int stage, int64_t *key);
int clair_host_train_set_sample(const int64_t *positions, int64_t n, const int64_t *truth, int64_t n_truth, double p_near, double p_outside, int64_t key,
                                uint8_t *cls, uint64_t *draws, uint8_t *sampled, int64_t *n_near, int64_t *n_outside);
int clair_host_train_set_pair_count(const int64_t *centres, int64_t n, const int64_t *truth, int64_t n_truth, const int64_t *bed_start, const int64_t *bed_end,
                                    int64_t n_bed, int64_t *v, int64_t *c);
int clair_host_train_set_ratio(int64_t v, double amp, int64_t c, double *r);
int clair_host_train_set_pair_keep(const int64_t *centres, int64_t n, const int64_t *truth, int64_t n_truth, const int64_t *bed_start, const int64_t *bed_end,
                                   int64_t n_bed, double r, int64_t key, int64_t *kept, int64_t *n_kept_var, int64_t *n_kept_non);
int clair_host_train_set_labels(const int64_t *centres, const uint8_t *centre_base, int64_t n, const int64_t *truth, const uint8_t *truth_labels, int64_t n_truth,
                                const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, uint8_t *labels, uint8_t *in_set);

/* -- the host twin of compare_vcf on the device (hostsrc/host_compare.cpp; docs/compare_vcf.md), with the rule of csrc/compare_core.h, the
 *    code the GPU runs inside clair_compare_* (include/clair_amd.h): the same entry points with the same arguments, statistics, counter
 *    block (CLAIR_COMPARE_COUNTS int64) and 32-byte records, as sequential loops.  The text handed to _parse is borrowed, not copied: it
 *    must stay where it is until the handle is destroyed or the side is parsed again.  Messages go to clair_host_last_error. */
typedef struct clair_host_compare clair_host_compare_t;
#ifndef CLAIR_COMPARE_RECORD_T
#define CLAIR_COMPARE_RECORD_T
typedef struct clair_compare_record clair_compare_record_t;
#endif
int clair_host_compare_create(clair_host_compare_t **out);
void clair_host_compare_destroy(clair_host_compare_t *h);
int clair_host_compare_set_contigs(clair_host_compare_t *h, const uint8_t *names, const int64_t *offsets, int n_contigs);
int clair_host_compare_set_regions(clair_host_compare_t *h, const int64_t *first, const int64_t *starts, const int64_t *ends, int64_t n_intervals);
int clair_host_compare_parse(clair_host_compare_t *h, int side, const uint8_t *text, int64_t len, int64_t *stats);
int clair_host_compare_keys(clair_host_compare_t *h, int side, int64_t *keys);
int clair_host_compare_permute(clair_host_compare_t *h, int side, const int64_t *perm);
int clair_host_compare_run(clair_host_compare_t *h);
int clair_host_compare_counts(clair_host_compare_t *h, int64_t *counts);
int clair_host_compare_records(clair_host_compare_t *h, int side, clair_compare_record_t *records, uint8_t *outcomes);
/* left alignment, as clair_compare_set_reference / _left_align / _allele_text; the reference is borrowed like the texts */
int clair_host_compare_set_reference(clair_host_compare_t *h, const uint8_t *seq, const int64_t *offsets, int n_contigs);
int clair_host_compare_left_align(clair_host_compare_t *h, int side, int64_t *stats);
int clair_host_compare_allele_text(clair_host_compare_t *h, int side, uint8_t *out);

/* -- index_bam on the CPU (hostsrc/host_bam_index.cpp; docs/index_bam.md): the host twin of clair_bamidx_* (include/clair_amd.h) with the
 *    rules of csrc/bam_index_core.h, and the file driver both backends run under.
 *    _create .. _backend: the twin, the same calls with the same arguments and results; blocks are inflated by zlib on `threads` threads,
 *      records framed by the sequential walk (segment_bytes 0) or by the segmented rule the device runs, restated (a power of two in 64 .. 8192).
 *    _debug_frame: the framing alone, as clair_bamidx_debug_frame: segment_bytes 0 is the walk.
 *    _build: the whole file through a backend: the BAM header (zlib), the BGZF block headers, batches of max_blocks blocks, the runs joined
 *      across batches, the order and the end of the file checked.  -> a result: _result_info [6] = references, records, mapped, unplaced, runs,
 *      windows of the linear index; _result_copy: the runs, the linear index (all-ones: an untouched window) and each reference's first window
 *      (n_ref + 1 words).  Writing the .bai from these is clair_amd/index_bam.py.
 *    Messages go to clair_host_last_error. */
typedef struct clair_host_bamidx clair_host_bamidx_t;
typedef struct clair_host_bamidx_result clair_host_bamidx_result_t;
#ifndef CLAIR_BAMIDX_TYPES
#define CLAIR_BAMIDX_TYPES
/* one run of records next to each other in the file that share (tid, bin): one chunk of a .bai, [beg, end) as virtual offsets */
typedef struct clair_bamidx_run {
    int32_t tid;
    uint32_t bin;
    uint64_t beg, end;
} clair_bamidx_run_t;      /* 24 bytes */
/* the batch interface of an index build, as the file driver (clair_host_bamidx_build) calls it: the entry points of one backend with its handle */
typedef struct clair_bamidx_backend {
    void *ctx;
    int (*begin)(void *ctx, int n_ref, const int64_t *ref_len);
    int (*batch)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                 const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state, const clair_bamidx_run_t **runs);
    int (*finish)(void *ctx, uint64_t *linear, int64_t n_windows, int64_t *counts);
    const char *(*last_error)(const void *ctx);
} clair_bamidx_backend_t;
#define CLAIR_BAMIDX_STATE 8   /* int64 words of `state`: in 0 records before the batch, 1 2 tid and pos of the record before it (0, INT32_MIN: none);
                                * out 3 records, 4 runs, 5 6 tid and pos of the last record (1 2 when there is none), 7 bytes carried over */
#endif
int clair_host_bamidx_create(int threads, int max_blocks, int segment_bytes, clair_host_bamidx_t **out);
void clair_host_bamidx_destroy(clair_host_bamidx_t *h);
int clair_host_bamidx_begin(clair_host_bamidx_t *h, int n_ref, const int64_t *ref_len);
int clair_host_bamidx_batch(clair_host_bamidx_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                            const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state,
                            const clair_bamidx_run_t **runs);
int clair_host_bamidx_finish(clair_host_bamidx_t *h, uint64_t *linear, int64_t n_windows, int64_t *counts);
int clair_host_bamidx_backend(clair_host_bamidx_t *h, clair_bamidx_backend_t *out);
int clair_host_bamidx_debug_frame(const uint8_t *stream, int64_t n, int64_t entry, int segment_bytes, int64_t *starts, int64_t cap, int64_t *result);
int clair_host_bamidx_build(const char *path, const clair_bamidx_backend_t *backend, int max_blocks, clair_host_bamidx_result_t **out);
int clair_host_bamidx_result_info(const clair_host_bamidx_result_t *r, int64_t *info);
int clair_host_bamidx_result_copy(const clair_host_bamidx_result_t *r, clair_bamidx_run_t *runs, uint64_t *linear, int64_t *first_window);
void clair_host_bamidx_result_free(clair_host_bamidx_result_t *r);

/* -- the input of the tools that rewrite a BAM, as a job (hostsrc/host_bam_job.cpp, hostsrc/bam_job.h): what clair_host_bamsort_run and
 *    clair_host_markdup_run read.
 *    _open: the BAM header of `path` read and checked -> a job; _header: its bytes as they are in the file (magic, text, reference list;
 *      *bytes is their length, copied when cap has room); _close.
 *    Messages go to clair_host_last_error. */
typedef struct clair_host_bam_job clair_host_bam_job_t;
int clair_host_bam_job_open(const char *path, clair_host_bam_job_t **out);
void clair_host_bam_job_close(clair_host_bam_job_t *job);
int clair_host_bam_job_header(const clair_host_bam_job_t *job, uint8_t *out, int64_t cap, int64_t *bytes);

/* -- sort_bam on the CPU (hostsrc/host_bam_sort.cpp; docs/sort_bam.md): the host twin of clair_bamsort_* (include/clair_amd.h) with the rules
 *    of csrc/bam_sort_core.h, and the file driver both backends run under.
 *    _create .. _backend, _debug_sort, _debug_gather: the twin, the same calls with the same arguments and results; blocks are inflated by
 *      zlib on `threads` threads, the group is ordered by std::stable_sort, `compressed` payloads are compressed by clair_host_deflate_bgzf.
 *    _run: the records of a job's file (clair_host_bam_job_open) sorted through a backend and appended to out_path (which holds the
 *      header's blocks already), the EOF marker behind them.  deflate: 0 the backend's own compressor, 1 zlib level 6, 2 clair_host_deflate_bgzf here.  memory: the most
 *      record bytes held at once.  stats [CLAIR_BAMSORT_STATS].
 *    Messages go to clair_host_last_error. */
typedef struct clair_host_bamsort clair_host_bamsort_t;
#ifndef CLAIR_BAMSORT_TYPES
#define CLAIR_BAMSORT_TYPES
/* the interface of a sort, as the file driver (clair_host_bamsort_run) calls it: the entry points of one backend with its handle */
typedef struct clair_bamsort_backend {
    void *ctx;
    int (*begin)(void *ctx, int n_ref, const int64_t *ref_len, int64_t memory);
    int (*pass)(void *ctx, int64_t bucket_lo, int64_t bucket_hi, int first);
    int (*batch)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                 const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
    int (*histogram)(void *ctx, int64_t *bytes, int64_t n_buckets);
    int (*sort)(void *ctx, int last, int64_t *info);
    int (*emit)(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
    const char *(*last_error)(const void *ctx);
} clair_bamsort_backend_t;
#define CLAIR_BAMSORT_STATE 11 /* int64 words of `state`: in 0 records before the batch, 1 the key of the record before it (0: none); out 2 records,
                                * 3 the last record's key (1 when there is none), 4 5 records and bytes kept for the group, 6 a record came before
                                * its predecessor, 7 the group outgrew `memory` and was dropped (first read only), 8 9 mapped and unplaced records,
                                * 10 bytes carried over */
#define CLAIR_BAMSORT_INFO 4   /* int64 words of _sort's `info`: bytes in the sorted buffer, payloads ready for _emit, records sorted, radix passes run */
#define CLAIR_BAMSORT_STATS 7  /* of clair_host_bamsort_run: records, mapped, unplaced, groups, reads of the input, already sorted, bytes appended */
#endif
int clair_host_bamsort_create(int threads, int max_blocks, int segment_bytes, clair_host_bamsort_t **out);
void clair_host_bamsort_destroy(clair_host_bamsort_t *h);
int clair_host_bamsort_begin(clair_host_bamsort_t *h, int n_ref, const int64_t *ref_len, int64_t memory);
int clair_host_bamsort_pass(clair_host_bamsort_t *h, int64_t bucket_lo, int64_t bucket_hi, int first);
int clair_host_bamsort_batch(clair_host_bamsort_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                             const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
int clair_host_bamsort_histogram(clair_host_bamsort_t *h, int64_t *bytes, int64_t n_buckets);
int clair_host_bamsort_sort(clair_host_bamsort_t *h, int last, int64_t *info);
int clair_host_bamsort_emit(clair_host_bamsort_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
int clair_host_bamsort_backend(clair_host_bamsort_t *h, clair_bamsort_backend_t *out);
int clair_host_bamsort_debug_sort(const uint64_t *keys, int64_t n, uint32_t *perm);
int clair_host_bamsort_debug_gather(const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, const uint32_t *perm, int64_t n, uint8_t *out,
                                    int64_t out_bytes);
int clair_host_bamsort_run(clair_host_bam_job_t *job, const clair_bamsort_backend_t *backend, const char *out_path, int deflate, int64_t memory,
                           int max_blocks, int threads, int64_t *stats);

/* -- markdup_bam on the CPU (hostsrc/host_markdup.cpp; docs/markdup_bam.md): the host twin of clair_markdup_* (include/clair_amd.h) with the
 *    rule of csrc/markdup_core.h, and the file driver both backends run under.
 *    _create .. _backend, _debug_summary, _debug_resolve: the twin, the same calls with the same arguments and results; blocks are inflated
 *      by zlib on `threads` threads, the resolution orders by std::stable_sort, `compressed` payloads are compressed by clair_host_deflate_bgzf.
 *    _run: two reads of a job's file (clair_host_bam_job_open) through a backend: every record summarised, the rule resolved, the
 *      records -- flagged, or with remove != 0 without the flagged ones -- appended to out_path (which holds the header's blocks already), the EOF marker behind them.
 *      deflate: 0 the backend's own compressor, 1 zlib level 6, 2 clair_host_deflate_bgzf here.  memory: the most bytes the summaries may
 *      hold.  stats [CLAIR_MARKDUP_STATS].
 *    Messages go to clair_host_last_error. */
typedef struct clair_host_markdup clair_host_markdup_t;
#ifndef CLAIR_MARKDUP_TYPES
#define CLAIR_MARKDUP_TYPES
typedef struct clair_markdup_summary {
    uint64_t end;   /* tid << 33 | (unclipped 5' position + 2^31) << 1 | reverse strand; all ones: the record is not examined */
    uint64_t hash;  /* FNV-1a (64 bit) of the read name without its NUL */
    uint32_t score; /* sum of the base qualities >= 15, clamped */
    uint32_t index; /* of the record in the file */
    uint32_t bits;  /* 1 examined, 2 can have a mate, 4 read 2 (else read 1), 8 reverse strand */
    uint32_t pad;
} clair_markdup_summary_t;
/* the interface of the stage, as the file driver (clair_host_markdup_run) calls it: the entry points of one backend with its handle */
typedef struct clair_markdup_backend {
    void *ctx;
    int (*begin)(void *ctx, int n_ref, int64_t memory, int remove);
    int (*batch)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                 const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
    int (*resolve)(void *ctx);
    int (*mark)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *info);
    int (*emit)(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
    int (*stats)(void *ctx, int64_t *counts);
    const char *(*last_error)(const void *ctx);
} clair_markdup_backend_t;
#define CLAIR_MARKDUP_STATE 3  /* int64 words of _batch's `state`: records summarised so far, records of this batch, bytes carried over */
#define CLAIR_MARKDUP_INFO 4   /* of _mark's `info`: bytes in the output buffer, payloads ready for _emit, records of this batch, records written */
#define CLAIR_MARKDUP_COUNTS 6 /* of _stats: records, examined, pairs, fragments, duplicate pairs, duplicate fragments */
#define CLAIR_MARKDUP_STATS 9  /* of clair_host_markdup_run: the six counts, duplicate records, records written, bytes appended */
#endif
int clair_host_markdup_create(int threads, int max_blocks, int segment_bytes, clair_host_markdup_t **out);
void clair_host_markdup_destroy(clair_host_markdup_t *h);
int clair_host_markdup_begin(clair_host_markdup_t *h, int n_ref, int64_t memory, int remove);
int clair_host_markdup_batch(clair_host_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                             const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
int clair_host_markdup_resolve(clair_host_markdup_t *h);
int clair_host_markdup_mark(clair_host_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                            const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *info);
int clair_host_markdup_emit(clair_host_markdup_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
int clair_host_markdup_stats(clair_host_markdup_t *h, int64_t *counts);
int clair_host_markdup_backend(clair_host_markdup_t *h, clair_markdup_backend_t *out);
int clair_host_markdup_debug_summary(const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, int64_t n, int n_ref,
                                     clair_markdup_summary_t *out);
int clair_host_markdup_debug_resolve(const clair_markdup_summary_t *summaries, int64_t n, uint8_t *duplicate);
int clair_host_markdup_run(clair_host_bam_job_t *job, const clair_markdup_backend_t *backend, const char *out_path, int deflate, int64_t memory,
                           int max_blocks, int threads, int remove, int64_t *stats);

/* -- gVCF on the CPU (hostsrc/host_gvcf.cpp; docs/gvcf.md): the host twin of clair_frontend_position_tallies / _gvcf_blocks
 *    (include/clair_amd.h) with the rule of csrc/gvcf_core.h, and the block rows' text.
 *    _tally: adds one slab of the host packer (clair_host_sampack_slab) to tallies [n][7] = A C G T I D N of the 0-based positions
 *      [lo, lo + n): only alignments flagged for the search (CLAIR_READ_EVC) count, I and D once per operation at the base before it,
 *      exactly as fe_tally_kernel counts them (ExtractVariantCandidates.py:296-316).  *anomalies collects CLAIR_FE_SEQ_OVERRUN /
 *      _BAD_BASE (such a base is not counted).
 *    _blocks: the rule and a sequential segmentation over those tallies; arguments, results and verdicts (return 2) as
 *      clair_frontend_gvcf_blocks.  ref: the reference bytes of [ref0, ref0 + ref_len).
 *    _format: blocks [first, first + n) as VCF rows "CTG POS . REF <NON_REF> . . END=e GT:GQ:DP:MIN_DP:PL 0/0:gq:dp:min_dp:pl,pl,pl",
 *      row_offsets [n + 1] their starts in out; *out_len is the length needed, written only when it fits out_cap. */
#ifndef CLAIR_GVCF_TYPES
#define CLAIR_GVCF_TYPES
typedef struct clair_gvcf_block {
    int64_t start, end;      /* 0-based, half-open */
    uint32_t min_dp, dp;     /* the smallest DP of the block; floor(sum of DP / length) */
    int32_t gq;              /* the smallest GQ of the block */
    int32_t pl[3];           /* per genotype 0/0, 0/1, 1/1 the smallest PL of the block */
} clair_gvcf_block_t;        /* 40 bytes */
#endif
int clair_host_gvcf_tally(const struct clair_read *reads, int64_t n_reads, const struct clair_op *ops, int64_t n_ops, const uint8_t *seq, int64_t seq_bytes,
                          int64_t lo, int64_t n, uint32_t *tallies, uint32_t *anomalies);
int clair_host_gvcf_blocks(const uint32_t *tallies, int64_t lo, int64_t n, const uint8_t *ref, int64_t ref_len, int64_t ref0, int c_match, int c_err, int c_half,
                           const uint8_t *band_of_gq, const int64_t *iv_start, const int64_t *iv_end, int64_t n_iv, clair_gvcf_block_t *out, int64_t capacity,
                           int64_t *n_blocks);
int clair_host_gvcf_format(const clair_gvcf_block_t *blocks, int64_t first, int64_t n, const char *ctg_name, const uint8_t *ref, int64_t ref_len, int64_t ref0,
                           char *out, int64_t out_cap, int64_t *out_len, int64_t *row_offsets);

#ifdef __cplusplus
}
#endif
#endif
