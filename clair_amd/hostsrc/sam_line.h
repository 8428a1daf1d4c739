// One line of `samtools view` text as the three host stages read it (host_pileup.cpp: clair_pileup, clair_evc; host_sampack.cpp:
// clair_sampack), and the loop that hands them a buffer line by line.  Internal to hostsrc/: not part of include/, exports nothing.
// Everything is inline or a template: the tokeniser is on the single-threaded path the device front end waits for.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

// str.split() whitespace: space, \t, \n, \r, \v, \f (and the ASCII separators 0x1c-0x1f, which text records never hold)
inline bool is_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x1f); }

// QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ: the first ten fields of line.split() (CreateTensor.py:252-263)
struct SamLine {
    const char *col[10];
    size_t len[10];
};

enum SamSplit { SAM_SKIP, SAM_OK, SAM_ERROR };

// SAM_SKIP: an @ line; SAM_ERROR: clair_host_fail has the message
inline SamSplit split_sam_line(const char *p, const char *end, int64_t line_no, SamLine *out) {
    int n = 0;
    while (p < end && n < 10) {
        while (p < end && is_space((unsigned char)*p)) ++p;
        if (p >= end) break;
        const char *q = p;
        while (q < end && !is_space((unsigned char)*q)) ++q;
        out->col[n] = p;
        out->len[n] = (size_t)(q - p);
        ++n;
        p = q;
    }
    if (n == 0) { clair_host_fail("alignment line %lld is empty", (long long)line_no); return SAM_ERROR; }
    if (out->col[0][0] == '@') return SAM_SKIP;
    if (n < 10) { clair_host_fail("alignment line %lld has %d columns (11 expected)", (long long)line_no, n); return SAM_ERROR; }
    return SAM_OK;
}

// column k (0-based) as a signed decimal of at most 18 digits -> true, or false with the message set
inline bool sam_int(const SamLine &line, int k, int64_t line_no, int64_t *out) {
    const char *s = line.col[k], *e = s + line.len[k];
    bool neg = false;
    if (s < e && (*s == '-' || *s == '+')) { neg = *s == '-'; ++s; }
    if (s != e && e - s <= 18) {
        int64_t x = 0;
        for (; s < e && *s >= '0' && *s <= '9'; ++s) x = x * 10 + (*s - '0');
        if (s == e) { *out = neg ? -x : x; return true; }
    }
    clair_host_fail("alignment line %lld: column %d is not an integer", (long long)line_no, k + 1);
    return false;
}

// a read less than 55 % aligned is skipped by the candidate search (ExtractVariantCandidates.py:143-157)
inline bool mostly_clipped(int64_t soft, int64_t total) { return 1.0 - (double)soft / (double)(total + 1) < 0.55; }

// Whole lines of sam[0, len) to sink->add_line(begin, end, line number), counted in sink->lines_seen; a last line without its line end only
// when `final`.  An error leaves *bytes_consumed at the start of the failing line, which is not counted.
template <class Sink> int feed_lines(Sink *sink, const char *sam, int64_t len, int final, int64_t *bytes_consumed) {
    if (!sink || (!sam && len > 0) || !bytes_consumed) return clair_host_fail("bad argument");
    int64_t at = 0;
    while (at < len) {
        const char *nl = (const char *)memchr(sam + at, '\n', (size_t)(len - at));
        if (!nl && !final) break;
        const char *end = nl ? nl : sam + len;
        if (sink->add_line(sam + at, end, sink->lines_seen)) { *bytes_consumed = at; return 1; }
        ++sink->lines_seen;
        at = (nl ? nl + 1 : end) - sam;
    }
    *bytes_consumed = at;
    return 0;
}
