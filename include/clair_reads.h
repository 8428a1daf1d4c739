/* clair_reads.h -- packed alignments: what the host packer (include/clair_host.h: clair_host_sampack_*) hands the device front
 * end (include/clair_amd.h: clair_frontend_*).
 *
 * The reference's two pileup stages (dataPrepScripts/ExtractVariantCandidates.py:259-345, CreateTensor.py:251-373) each read
 * `samtools view` text and walk CIGAR and SEQ character by character.  Here the text is read ONCE; a slab holds, for the alignments
 * either stage would use, the columns both walk (POS, the strand bit of FLAG, SEQ upper-cased) and the CIGAR as a list of the
 * operations that touch a reference position or a read base in those loops: M/=/X, I, D.  S is folded into the read offset of the
 * next operation; H, N, P and anything else move neither cursor there (:296-316, :289-365) and are dropped.
 *
 * One "element" is one iteration of the innermost loops: a matched, inserted or deleted base.  Element e of a slab belongs to the
 * operation j with op_elem[j] <= e < op_elem[j+1] (exclusive prefix sum of the operation lengths, n_ops + 1 entries). */
#ifndef CLAIR_READS_H
#define CLAIR_READS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clair_read {
    int64_t pos0;        /* POS - 1 (CreateTensor.py:258) */
    uint32_t seq0;       /* first byte of SEQ in the slab's base array */
    uint32_t seq_len;
    uint32_t op0;        /* first operation in the slab's operation array */
    uint32_t n_ops;
    uint32_t flags;      /* CLAIR_READ_* */
    uint32_t reserved;   /* 0, unless the slab was packed for the indel look-up: CLAIR_READ_LOOKUP below */
} clair_read_t;          /* 32 bytes */

enum {
    CLAIR_READ_REVERSE = 1,   /* FLAG & 16 (CreateTensor.py:264) */
    CLAIR_READ_EVC = 2,       /* passes the candidate search's filters: RNAME, MQ, CIGAR != "*", >= 55 % aligned (EVC :279-293) */
    CLAIR_READ_PILE = 4,      /* walked by the pileup: in the pileup's region, MQ, not beyond --dcov at its start (CT :266-287) */
    CLAIR_READ_FLUSH = 8,     /* first read the pileup walks at a new start position: windows left of it are complete (CT :369) */
    CLAIR_READ_LOOKUP = 16    /* counted by the indel look-up (below): on the contig, with a CIGAR, whatever its MQ and its rank under --dcov.  Set
                               * only by a packer that was asked to (clair_host_sampack_set_lookup, clair_frontend_bam_lookup), which then also keeps
                               * the alignments neither stage walks; both stages ignore an alignment without EVC / PILE.  `reserved` of such an
                               * alignment marks the I / D operations that follow something the slab does not hold and that is no M / = / X (a P or
                               * H, a zero-length operation), and every I / D after an N -- the scripts' walk does not advance over an N, so the slab
                               * places what follows one where THEY see it, not where it lies: bit min(k, 31) for the alignment's k-th kept
                               * operation.  The look-up skips them. */
};

typedef struct clair_op {
    uint32_t read;       /* index of the alignment in the slab */
    uint32_t code_len;   /* length << 2 | code; lengths are > 0 */
    int32_t ref_off;     /* reference offset of the operation from pos0 */
    uint32_t q_off;      /* offset of its first base in the alignment's SEQ */
} clair_op_t;            /* 16 bytes */

enum { CLAIR_OP_M = 0, CLAIR_OP_I = 1, CLAIR_OP_D = 2 };

/* What takes a run out of the regime the device front end reproduces exactly (LABNOTES.md part B 6b); the caller then runs the sequential
 * host code (clair_host_evc_*, clair_host_pileup_*), which reproduces the reference there too, errors included. */
enum {
    CLAIR_FE_UNSORTED = 1,        /* start positions decrease */
    CLAIR_FE_ZERO_INDEL = 2,      /* "0I" / "0D": the candidate search counts the operation, there is no base to hang it on */
    CLAIR_FE_LONG_SPAN = 4,       /* reference span beyond len(SEQ) + 100 000: the reference has not loaded those candidates yet (CT :274) */
    CLAIR_FE_SEQ_OVERRUN = 8,     /* CIGAR walks past the end of SEQ: an IndexError in the reference */
    CLAIR_FE_BAD_BASE = 16,       /* a read base that is not an IUPAC code: KeyError in the candidate search, a skipped tuple in the pileup */
    CLAIR_FE_BAD_REF = 32,        /* reference base missing or not an IUPAC code under a walked position */
    CLAIR_FE_OVERFLOW = 64,       /* a count beyond int16 */
    CLAIR_FE_BUDGET = 128,        /* the budget of 5 M outstanding tuples would have run out (CT :181, 289): results depend on offer order */
    CLAIR_FE_CANDIDATES = 256,    /* a given candidate list is not strictly ascending */
    CLAIR_FE_LEAD_INDEL = 512     /* an alignment the candidate search accepts begins with an I or D (tallied at POS - 1) and an earlier accepted alignment has
                                   * the same POS: the reference flushed POS - 1 after that one (EVC :316-345: positions < POS after EVERY alignment) and
                                   * evaluates the late tally on its own, which one sum per position cannot reproduce */
};

/* ---- the indel look-up: "the most frequent inserted / deleted sequence right after position p" answered from the slabs ----------
 * (clair/call_var.py:78-170: insertion_bases_using_pysam_from / deletion_bases_using_pysam_from over pysam's pileup column p - 1.)
 * Per queried position (1-based p) the table of DISTINCT keys among the I / D operations that count at p: the operation belongs to a
 * CLAIR_READ_LOOKUP alignment, is 1 .. 50 long (CLAIR_LOOKUP_MAX_LEN: nothing longer is ever asked for, call_var.py:30), the kept
 * operation before it in the same alignment is an M that ends where it starts (so no N, P, H, I or D lies between, and it does not open
 * the alignment), and that M's last reference base is 0-based p - 1.  Key of an insertion: its bases, upper-cased; of a deletion: its
 * length.  Entries come in the order their key was first seen (ascending first_rank; rank = index of the alignment over all slabs in
 * feed order).  The caller applies min_len / max_len / ignore and takes the highest count, the first seen among equals -- the rule of
 * the reference's max(dict, key=dict.get).  depth = CLAIR_READ_LOOKUP alignments with an M or D over 0-based p - 1. */
#define CLAIR_LOOKUP_MAX_LEN 50
typedef struct clair_indel_entry {
    int8_t sign;             /* +1 insertion, -1 deletion */
    uint8_t length;          /* 1 .. CLAIR_LOOKUP_MAX_LEN */
    uint16_t reserved;       /* 0 */
    uint32_t count;          /* operations with this key */
    uint32_t first_rank;     /* rank of the first alignment that showed it */
    uint8_t bases[50];       /* insertion: its bases, zero-padded; deletion: zeros (the host slices the FASTA) */
    uint8_t pad[2];          /* 0 */
} clair_indel_entry_t;       /* 64 bytes */

enum {
    CLAIR_LOOKUP_HITS = 1,       /* device only: more operations counted at this position than the device's hit list holds per query (512), or two keys
                                  * shared a hash: the table of this query was computed by the host twin instead (same bytes) */
    CLAIR_LOOKUP_ENTRIES = 2     /* more distinct keys than `capacity`: n_entries is the number there are, the first `capacity` were written; ask again
                                  * with that capacity */
};

#ifdef __cplusplus
}
#endif
#endif
