// Host-side helpers of the Clair hot path (include/clair_host.h): BAM input without samtools (callVarBam --bam_reader native).
// Plain C++17 + zlib, no HIP.
//
// What `samtools view -F 2316 <bam> <region>` does before it formats text, restated for the one use this project makes of it:
//   - BGZF: which blocks a query reads and how many to a batch; the block format and the zlib inflate (N threads, each block's CRC32 and
//     ISIZE checked) are hostsrc/bgzf_file.h.  A missing EOF block is a warning (as htslib's); clair_host_bam_set_inflater hands the batches
//     of a query to another inflater instead (the device's: callVarBam --bam_inflate device);
//   - the BAM header (hostsrc/bam_header.h): the reference names and lengths;
//   - region selection with the .bai: bins overlapping the region, chunks before the linear index's minimum offset dropped, the rest
//     sorted and merged (htslib's hts_itr_query), or a scan from the first record without an index;
//   - the record walker: whole records, framed by the step every reader of records here takes (csrc/bam_record_core.h), the walk ending at
//     the first record of the contig that starts past the region (hts_itr_next).
// The binary records go to the device as they are (clair_frontend_add_bam, csrc/frontend.hip).  clair_host_bam_render turns them into the
// 11 mandatory columns samtools prints -- the text the host stages and the device front end's fall-back read; the size rule, the CIGAR
// span and the walk to the real CIGAR are csrc/bam_record_core.h, the device decoder's own -- and clair_host_faidx
// is `samtools faidx` for one region.  clair_host_bam_set_subsample adds `-s` to that view (csrc/subsample_core.h, docs/subsample.md).
#include "../../include/clair_host.h"
#include "../csrc/subsample_core.h"
#include "bam_header.h"
#include "bgzf_file.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace clair_rec;
using namespace clair_bgzf;

constexpr uint16_t VIEW_FILTER = 2316;       // shared/param.py:6: unmapped, mate unmapped, secondary, supplementary
const char NT16[] = "=ACMGRSVTWYHKDBN";
const char CIGAR_OPS[] = "MIDNSHP=XB??????";

inline int32_t i32(const uint8_t *p) { return (int32_t)u32(p); }
inline uint64_t u64(const uint8_t *p) { return (uint64_t)u32(p) | (uint64_t)u32(p + 4) << 32; }

struct Block {                               // one compressed block of a batch
    uint64_t coffset;
    uint32_t csize;                          // whole block, header and footer included
    size_t in_at;                            // where its bytes are in the batch's compressed buffer
    size_t out_at, out_len;                  // where its inflated bytes go
};

struct Chunk { uint64_t beg, end; };         // virtual offsets, [beg, end)

// what is wrong with the sizes of a record's fixed and variable parts or with its read name, or nullptr
const char *record_sizes(const uint8_t *r, uint32_t block_size) {
    const uint32_t l_read_name = r[12];
    int verdict = sizes_verdict(block_size, l_read_name, u16(r + 16), i32(r + 20));
    if (verdict == SIZES_OK && r[4 + 32 + l_read_name - 1] != 0) verdict = SIZES_NAME;
    return verdict == SIZES_OK ? nullptr : sizes_text(verdict);
}

// the record's CIGAR as `samtools view` prints it: the stored one, or the one in CG:B:I behind the kSmN placeholder.  r: after record_sizes
const uint8_t *printed_cigar(const uint8_t *r, uint32_t block_size, uint32_t *n_ops) {
    const uint32_t l_read_name = r[12], n_cigar = u16(r + 16);
    const int32_t ref_id = i32(r + 4), pos = i32(r + 8), l_seq = i32(r + 20);
    const uint64_t cigar = 36 + l_read_name;
    uint64_t cg = cigar;
    *n_ops = n_cigar;
    if (n_cigar > 0 && ref_id >= 0 && pos >= 0 && (u32(r + cigar) & 15) == 4 && (u32(r + cigar) >> 4) == (uint32_t)l_seq)
        real_cigar(Bytes{r}, cigar + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq, 4ull + block_size, n_cigar, &cg, n_ops);
    return r + cg;
}

void append_uint(std::string &s, uint64_t v) { char b[24]; int n = snprintf(b, sizeof b, "%llu", (unsigned long long)v); s.append(b, (size_t)n); }
void append_int(std::string &s, int64_t v) { char b[24]; int n = snprintf(b, sizeof b, "%lld", (long long)v); s.append(b, (size_t)n); }

}  // namespace

struct clair_bam {
    std::string path;
    FILE *file = nullptr;
    int threads = 4;
    size_t batch_blocks = 4;                 // blocks read and inflated at a time: few for the header, 64 per thread for records
    uint64_t file_size = 0;
    bool have_eof = true;
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    uint64_t first_record = 0;               // virtual offset of the first record (after the header)
    // the query being walked
    int tid = -1;
    int64_t beg0 = 0, end0 = INT64_MAX;      // 0-based half-open
    bool scanning = false, seen_tid = false, done = true, used_index = false;
    std::vector<Chunk> chunks;
    size_t chunk_at = 0;
    uint64_t next_coffset = 0;               // next block of the current chunk to read
    bool chunk_open = false;
    // inflated bytes not yet handed out (a partial record at the front) and the virtual offset of each block's first byte in it
    std::vector<uint8_t> pending;
    size_t pending_at = 0;
    std::vector<std::pair<size_t, uint64_t>> block_starts;   // (position in pending, virtual offset)
    std::vector<uint64_t> rec_voffset;       // per record of the last chunk handed out
    int64_t records = 0;
    std::string rendered;
    // batch buffers
    std::vector<uint8_t> cbuf;
    std::vector<Block> blocks;
    std::vector<uint8_t> obuf;
    // another inflater for the batches (clair_host_bam_set_inflater); none: zlib on `threads` threads.  hook_*: the batch as either takes it
    clair_host_inflate_fn inflater = nullptr;
    void *inflater_ctx = nullptr;
    std::vector<int64_t> hook_in_at, hook_out_at;
    std::vector<int32_t> hook_csize, hook_out_len, hook_status;
    // clair_host_bam_set_subsample: one more clause of render's view; frac <= 0: off
    uint32_t subsample_seed = 0;
    double subsample_frac = 0.0;

    ~clair_bam() { if (file) fclose(file); }

    int read_at(uint64_t off, uint8_t *dst, size_t n) {
        if (fseeko(file, (off_t)off, SEEK_SET) != 0) return -1;
        return fread(dst, 1, n, file) == n ? 0 : -1;
    }

    // reads the compressed blocks from `coffset` up to the stop block while the batch has room, and inflates them
    int read_blocks(uint64_t coffset, size_t max_blocks, uint64_t stop_coffset, bool include_stop) {
        blocks.clear();
        cbuf.clear();
        size_t out = 0;
        while (blocks.size() < max_blocks && (coffset < stop_coffset || (include_stop && coffset == stop_coffset)) && coffset < file_size) {
            uint32_t csize = 0, isize = 0;
            const size_t in_at = cbuf.size();
            if (read_block(file, path.c_str(), file_size, coffset, cbuf, &csize, &isize)) return 1;
            blocks.push_back(Block{coffset, csize, in_at, out, isize});
            out += isize;
            coffset += csize;
        }
        next_coffset = coffset;
        obuf.resize(out + 1);
        return blocks.empty() ? 0 : inflate_batch();
    }

    // the batch through zlib on `threads` threads or through the installed inflater; the first block with a status says what it is
    int inflate_batch() {
        const size_t n = blocks.size();
        hook_in_at.resize(n); hook_out_at.resize(n); hook_csize.resize(n); hook_out_len.resize(n);
        hook_status.assign(n, 0);
        for (size_t i = 0; i < n; ++i) {
            hook_in_at[i] = (int64_t)blocks[i].in_at;
            hook_csize[i] = (int32_t)blocks[i].csize;
            hook_out_at[i] = (int64_t)blocks[i].out_at;
            hook_out_len[i] = (int32_t)blocks[i].out_len;
        }
        if (!inflater)
            inflate_blocks(threads, cbuf.data(), (int)n, hook_in_at.data(), hook_csize.data(), hook_out_at.data(), hook_out_len.data(), obuf.data(), hook_status.data());
        else if (inflater(inflater_ctx, cbuf.data(), (int64_t)cbuf.size(), (int)n, hook_in_at.data(), hook_csize.data(), hook_out_at.data(), hook_out_len.data(),
                          obuf.data(), hook_status.data()) != 0)
            return clair_host_fail("%s: the installed inflater failed on the %zu blocks from compressed offset %llu", path.c_str(), n,
                                   (unsigned long long)blocks[0].coffset);
        for (size_t i = 0; i < n; ++i)
            if (hook_status[i] != 0)
                return clair_host_fail("%s: BGZF block at compressed offset %llu: %s", path.c_str(), (unsigned long long)blocks[i].coffset, inflate_text(hook_status[i]));
        return 0;
    }

    // more inflated bytes of the current chunk onto `pending`; *got = 0 when the chunks are exhausted
    int fill(size_t *got) {
        *got = 0;
        while (chunk_at < chunks.size()) {
            const Chunk &c = chunks[chunk_at];
            if (!chunk_open) { next_coffset = c.beg >> 16; chunk_open = true; }
            const uint64_t stop = c.end >> 16;
            const bool include_stop = (c.end & 0xffff) != 0;
            if (!(next_coffset < stop || (include_stop && next_coffset == stop)) || next_coffset >= file_size) {
                chunk_open = false;
                ++chunk_at;
                continue;
            }
            if (read_blocks(next_coffset, batch_blocks, stop, include_stop)) return 1;
            if (pending_at > 0) {                // drop what was handed out
                pending.erase(pending.begin(), pending.begin() + (ptrdiff_t)pending_at);
                for (auto &bs : block_starts) {
                    if (bs.first >= pending_at) { bs.first -= pending_at; continue; }
                    bs.second += pending_at - bs.first;      // the block's bytes from pending_at on: same block, larger in-block offset
                    bs.first = 0;
                }
                pending_at = 0;
            }
            while (block_starts.size() > 1 && block_starts[1].first == 0) block_starts.erase(block_starts.begin());
            for (const Block &b : blocks) {
                size_t from = 0, to = b.out_len;
                if (b.coffset == (c.beg >> 16)) from = std::min<size_t>(c.beg & 0xffff, to);
                if (b.coffset == stop && include_stop) to = std::min<size_t>(c.end & 0xffff, to);
                if (to <= from) continue;
                block_starts.emplace_back(pending.size(), b.coffset << 16 | from);
                pending.insert(pending.end(), obuf.begin() + (ptrdiff_t)(b.out_at + from), obuf.begin() + (ptrdiff_t)(b.out_at + to));
                *got += to - from;
            }
            if (*got) return 0;
        }
        return 0;
    }

    uint64_t voffset_at(size_t pos) const {
        auto it = std::upper_bound(block_starts.begin(), block_starts.end(), std::make_pair(pos, UINT64_MAX));
        if (it == block_starts.begin()) return 0;
        --it;
        return it->second + (pos - it->first);
    }
};

extern "C" {

int clair_host_bam_open(const char *path, int threads, clair_bam_t **out) {
    if (!out) return clair_host_fail("out is NULL");
    *out = nullptr;
    if (!path) return clair_host_fail("no BAM path");
    if (threads < 1 || threads > 16) return clair_host_fail("BAM threads: %d (1 .. 16)", threads);
    clair_bam *b = new clair_bam;
    b->path = path;
    b->threads = threads;
    auto bail = [&](int rc) { delete b; return rc; };
    b->file = fopen(path, "rb");
    if (!b->file) return bail(clair_host_fail("%s: cannot open", path));
    if (fseeko(b->file, 0, SEEK_END) != 0) return bail(clair_host_fail("%s: cannot seek", path));
    b->file_size = (uint64_t)ftello(b->file);
    uint8_t magic[BGZF_HEADER] = {0};
    if (b->file_size < BGZF_HEADER || b->read_at(0, magic, BGZF_HEADER) || !gzip_with_extra(magic) || !bc_subfield(magic))
        return bail(clair_host_fail("%s is not a BGZF-compressed BAM (SAM text, CRAM and plain gzip are read by samtools): use --bam_reader samtools", path));
    if (b->file_size >= 28) {
        uint8_t tail[28];
        b->have_eof = !b->read_at(b->file_size - 28, tail, 28) && !memcmp(tail, BGZF_EOF, 28);
    } else {
        b->have_eof = false;
    }
    // the header: inflate from the start until it is complete
    b->chunks.assign(1, Chunk{0, UINT64_MAX});
    b->chunk_at = 0;
    b->chunk_open = false;
    auto need = [&](size_t n) -> int {
        while (b->pending.size() - b->pending_at < n) {
            size_t got = 0;
            if (b->fill(&got)) return 1;
            if (!got) return clair_host_fail("%s: the BAM header is truncated", path);
        }
        return 0;
    };
    BamHeader header;
    if (parse_bam_header(path, ": use --bam_reader samtools", need, [&] { return (const uint8_t *)b->pending.data(); }, &header)) return bail(1);
    b->names.swap(header.names);
    b->lengths.swap(header.lengths);
    b->first_record = b->voffset_at(header.end);
    b->batch_blocks = (size_t)std::max(16, 64 * threads);
    b->pending.clear();
    b->pending_at = 0;
    b->block_starts.clear();
    b->done = true;
    *out = b;
    return 0;
}

void clair_host_bam_close(clair_bam_t *b) { delete b; }

int clair_host_bam_set_inflater(clair_bam_t *b, clair_host_inflate_fn fn, void *ctx, int batch_blocks) {
    if (!b) return clair_host_fail("BAM handle is NULL");
    if (fn && (batch_blocks < 1 || batch_blocks > 16384)) return clair_host_fail("inflater batch of %d blocks: 1 .. 16384", batch_blocks);
    b->inflater = fn;
    b->inflater_ctx = fn ? ctx : nullptr;
    b->batch_blocks = fn ? (size_t)batch_blocks : (size_t)std::max(16, 64 * b->threads);
    return 0;
}

int clair_host_bam_set_subsample(clair_bam_t *b, int64_t seed, double frac) {
    if (!b) return clair_host_fail("BAM handle is NULL");
    if (seed < 0 || seed > 0xffffffffll) return clair_host_fail("subsample seed %lld: 0 .. 4294967295", (long long)seed);
    b->subsample_seed = (uint32_t)seed;
    b->subsample_frac = frac > 0.0 ? frac : 0.0;
    return 0;
}

int clair_host_subsample_keeps(const uint8_t *name, int64_t n, int64_t seed, double frac) {
    if (n < 0 || (n > 0 && !name) || seed < 0 || seed > 0xffffffffll) { clair_host_fail("subsample_keeps: bad name or seed"); return -1; }
    const int64_t len = n > 0 ? (int64_t)strnlen((const char *)name, (size_t)n) : 0;
    return subsample_keeps(subsample_hash(name, len), (uint32_t)seed, frac) ? 1 : 0;
}

int clair_host_bam_info(const clair_bam_t *b, int64_t *info) {
    if (!b || !info) return clair_host_fail("NULL argument");
    info[0] = (int64_t)b->names.size();
    info[1] = b->have_eof ? 1 : 0;
    info[2] = b->records;
    info[3] = b->used_index ? 1 : 0;
    return 0;
}

int clair_host_bam_ref(const clair_bam_t *b, int tid, const char **name, int64_t *length) {
    if (!b || tid < 0 || tid >= (int)b->names.size()) return clair_host_fail("reference id %d out of range", tid);
    if (name) *name = b->names[(size_t)tid].c_str();
    if (length) *length = b->lengths[(size_t)tid];
    return 0;
}

int clair_host_bam_tid(const clair_bam_t *b, const char *name) {
    if (!b || !name) return -1;
    for (size_t i = 0; i < b->names.size(); ++i)
        if (b->names[i] == name) return (int)i;
    return -1;
}

int clair_host_bam_query(clair_bam_t *b, const char *index_path, int tid, int64_t beg1, int64_t end1) {
    if (!b) return clair_host_fail("BAM handle is NULL");
    if (tid < 0 || tid >= (int)b->names.size()) return clair_host_fail("reference id %d is not in the BAM header", tid);
    b->tid = tid;
    const bool whole = beg1 < 0 || end1 < 0;
    b->beg0 = whole ? 0 : std::max<int64_t>(beg1 - 1, 0);
    b->end0 = whole ? INT64_MAX : end1;
    b->chunks.clear();
    b->pending.clear();
    b->pending_at = 0;
    b->block_starts.clear();
    b->chunk_at = 0;
    b->chunk_open = false;
    b->seen_tid = false;
    b->records = 0;
    b->done = false;
    b->used_index = index_path != nullptr;
    b->scanning = !b->used_index;
    if (!b->used_index) {
        b->chunks.push_back(Chunk{b->first_record, UINT64_MAX});
        return 0;
    }
    FILE *f = fopen(index_path, "rb");
    if (!f) return clair_host_fail("%s: cannot open", index_path);
    std::vector<uint8_t> idx;
    {
        uint8_t tmp[1 << 16];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) idx.insert(idx.end(), tmp, tmp + n);
        fclose(f);
    }
    size_t at = 0;
    auto take = [&](size_t n) -> const uint8_t * {
        if (at + n > idx.size()) return nullptr;
        const uint8_t *p = idx.data() + at;
        at += n;
        return p;
    };
    const uint8_t *p = take(8);
    if (!p || memcmp(p, "BAI\1", 4)) return clair_host_fail("%s is not a BAI index", index_path);
    const int32_t n_ref = i32(p + 4);
    if (n_ref != (int32_t)b->names.size()) return clair_host_fail("%s lists %d references, the BAM header %zu", index_path, n_ref, b->names.size());
    // region in BAI coordinates: bins of [beg, end) with end capped at 2^29 (the binning scheme's extent)
    const int64_t beg = b->beg0, end = std::min<int64_t>(b->end0, (int64_t)1 << 29);
    std::vector<Chunk> chunks;
    uint64_t min_off = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        if (!(p = take(4))) return clair_host_fail("%s is truncated", index_path);
        const int32_t n_bin = i32(p);
        for (int32_t k = 0; k < n_bin; ++k) {
            if (!(p = take(8))) return clair_host_fail("%s is truncated", index_path);
            const uint32_t bin = u32(p);
            const int32_t n_chunk = i32(p + 4);
            if (n_chunk < 0 || !(p = take((size_t)n_chunk * 16))) return clair_host_fail("%s is truncated", index_path);
            if (r != tid || bin > 37449 || beg >= end) continue;     // 37450: the pseudo-bin of per-reference counts
            // bin -> its level and range (reg2bins restated): first bins of levels 0..5 are 0, 1, 9, 73, 585, 4681
            static const uint32_t first[6] = {0, 1, 9, 73, 585, 4681};
            int level = 5;
            while (level > 0 && bin < first[level]) --level;
            const int shift = 29 - 3 * level;
            const int64_t lo = (int64_t)(bin - first[level]) << shift, hi = lo + ((int64_t)1 << shift);
            if (hi <= beg || lo >= end) continue;
            for (int32_t c = 0; c < n_chunk; ++c) chunks.push_back(Chunk{u64(p + 16 * c), u64(p + 16 * c + 8)});
        }
        if (!(p = take(4))) return clair_host_fail("%s is truncated", index_path);
        const int32_t n_intv = i32(p);
        if (n_intv < 0 || !(p = take((size_t)n_intv * 8))) return clair_host_fail("%s is truncated", index_path);
        if (r == tid && n_intv > 0) {
            const int64_t w = std::min<int64_t>(beg >> 14, n_intv - 1);
            min_off = u64(p + 8 * w);
            for (int64_t j = w; j >= 0 && min_off == 0; --j) min_off = u64(p + 8 * j);   // empty windows carry 0
        }
    }
    std::vector<Chunk> kept;
    for (const Chunk &c : chunks)
        if (c.end > min_off) kept.push_back(c);
    std::sort(kept.begin(), kept.end(), [](const Chunk &a, const Chunk &c) { return a.beg < c.beg; });
    for (const Chunk &c : kept) {                // merge what overlaps or touches: every record is read once, in file order
        if (!b->chunks.empty() && c.beg <= b->chunks.back().end) b->chunks.back().end = std::max(b->chunks.back().end, c.end);
        else b->chunks.push_back(c);
    }
    if (b->chunks.empty()) b->done = true;
    return 0;
}

int clair_host_bam_next(clair_bam_t *b, uint8_t *buf, int64_t cap, int64_t *offsets, int64_t max_records, int64_t *len, int64_t *n_records) {
    if (!b || !buf || !offsets || !len || !n_records) return clair_host_fail("NULL argument");
    *len = 0;
    *n_records = 0;
    b->rec_voffset.clear();
    int64_t fill = 0, n = 0;
    while (!b->done && n < max_records) {
        int64_t next = 0;
        const int rc = step(Bytes{b->pending.data()}, (int64_t)b->pending_at, (int64_t)b->pending.size(), &next);
        char why[200];
        if (rc == STEP_PAST) {                                   // the record is not all here yet
            size_t got = 0;
            if (b->fill(&got)) return 1;
            if (got) continue;
            if (b->pending.size() > b->pending_at) {
                describe_cut(why, sizeof why, b->voffset_at(b->pending_at));
                return clair_host_fail("%s: %s", b->path.c_str(), why);
            }
            b->done = true;
            break;
        }
        const uint8_t *r = b->pending.data() + b->pending_at;
        const uint32_t block_size = u32(r);
        const uint64_t voff = b->voffset_at(b->pending_at);
        if (rc == STEP_BAD) {
            describe_bad_step(why, sizeof why, voff, block_size);
            return clair_host_fail("%s: %s", b->path.c_str(), why);
        }
        const int32_t ref_id = i32(r + 4), pos = i32(r + 8);
        if (ref_id == b->tid) {
            b->seen_tid = true;
            if (pos >= b->end0) { b->done = true; break; }       // hts_itr_next: the first record past the region ends the walk
        } else if (b->seen_tid || !b->scanning) {
            b->done = true;                                      // sorted input: the contig's records are behind
            break;
        } else {                                                 // a scan before the contig starts: skip
            b->pending_at += 4 + (size_t)block_size;
            continue;
        }
        if (fill + 4 + (int64_t)block_size > cap) {
            if (n == 0) return clair_host_fail("%s: a record of %u bytes does not fit a chunk of %lld", b->path.c_str(), block_size + 4, (long long)cap);
            break;
        }
        memcpy(buf + fill, r, 4 + (size_t)block_size);
        offsets[n++] = fill;
        b->rec_voffset.push_back(voff);
        fill += 4 + (int64_t)block_size;
        b->pending_at += 4 + (size_t)block_size;
    }
    b->records += n;
    *len = fill;
    *n_records = n;
    return 0;
}

int clair_host_bam_voffset(const clair_bam_t *b, int64_t k, uint64_t *voffset) {
    if (!b || !voffset || k < 0 || k >= (int64_t)b->rec_voffset.size()) return clair_host_fail("record %lld is not in the last chunk", (long long)k);
    *voffset = b->rec_voffset[(size_t)k];
    return 0;
}

int clair_host_bam_render(clair_bam_t *b, const uint8_t *records, const int64_t *offsets, int64_t n, int tid, int64_t beg1, int64_t end1,
                          const char **text, int64_t *len) {
    if (!b || !text || !len || (n > 0 && (!records || !offsets))) return clair_host_fail("NULL argument");
    std::string &s = b->rendered;
    s.clear();
    const bool whole = beg1 < 0 || end1 < 0;
    for (int64_t k = 0; k < n; ++k) {
        const uint8_t *r = records + offsets[k];
        const uint32_t block_size = u32(r);
        if (block_size < 32) return clair_host_fail("record %lld: block_size %u < 32", (long long)k, block_size);
        if (const char *why = record_sizes(r, block_size)) return clair_host_fail("record %lld: %s", (long long)k, why);
        const int32_t ref_id = i32(r + 4), pos = i32(r + 8), next_ref = i32(r + 24), next_pos = i32(r + 28), tlen = i32(r + 32);
        const uint32_t l_read_name = r[12], mapq = r[13], n_cigar_stored = u16(r + 16), flag = u16(r + 18);
        const int32_t l_seq = i32(r + 20);
        uint32_t n_cigar = 0;
        const uint8_t *cigar = printed_cigar(r, block_size, &n_cigar);
        // `samtools view -F 2316 <bam> <region>`
        if (flag & VIEW_FILTER) continue;
        if (ref_id != tid) continue;
        if (!whole) {
            int64_t rlen = (flag & 4) ? 0 : cigar_span(Bytes{cigar}, 0, n_cigar);
            if (rlen == 0) rlen = 1;
            const int64_t end_1 = (int64_t)pos + rlen;           // bam_endpos, 1-based inclusive
            if (!((int64_t)pos + 1 <= end1 && end_1 >= beg1)) continue;
        }
        if (b->subsample_frac > 0.0
            && !subsample_keeps(subsample_hash(r + 36, (int64_t)strnlen((const char *)r + 36, l_read_name - 1)), b->subsample_seed, b->subsample_frac))
            continue;
        const auto ref_name = [&](int32_t id) -> const std::string * {
            return id >= 0 && id < (int32_t)b->names.size() ? &b->names[(size_t)id] : nullptr;
        };
        if (ref_id >= 0 && !ref_name(ref_id)) return clair_host_fail("record %lld: reference id %d is not in the header", (long long)k, ref_id);
        s.append((const char *)r + 36, l_read_name - 1);
        s += '\t'; append_uint(s, flag);
        s += '\t'; s += ref_id < 0 ? std::string("*") : *ref_name(ref_id);
        s += '\t'; append_int(s, (int64_t)pos + 1);
        s += '\t'; append_uint(s, mapq);
        s += '\t';
        if (n_cigar == 0) s += '*';
        for (uint32_t i = 0; i < n_cigar; ++i) { const uint32_t c = u32(cigar + 4ull * i); append_uint(s, c >> 4); s += CIGAR_OPS[c & 15]; }
        s += '\t';
        if (next_ref < 0) s += '*';
        else if (next_ref == ref_id) s += '=';
        else if (const std::string *nm = ref_name(next_ref)) s += *nm;
        else return clair_host_fail("record %lld: mate reference id %d is not in the header", (long long)k, next_ref);
        s += '\t'; append_int(s, (int64_t)next_pos + 1);
        s += '\t'; append_int(s, tlen);
        s += '\t';
        const uint8_t *seq = r + 36 + l_read_name + 4ull * n_cigar_stored, *qual = seq + ((uint64_t)l_seq + 1) / 2;
        if (l_seq == 0) s += '*';
        for (int32_t i = 0; i < l_seq; ++i) s += NT16[(seq[i >> 1] >> ((~i & 1) << 2)) & 15];
        s += '\t';
        if (l_seq == 0 || qual[0] == 0xff) s += '*';
        else for (int32_t i = 0; i < l_seq; ++i) s += (char)(qual[i] + 33);
        s += '\n';
    }
    *text = s.data();
    *len = (int64_t)s.size();
    return 0;
}

int clair_host_faidx(const char *fasta, const char *ctg, int64_t beg1, int64_t end1, char *out, int64_t cap, int64_t *len) {
    if (!fasta || !ctg || !len) return clair_host_fail("NULL argument");
    const std::string fai = std::string(fasta) + ".fai";
    FILE *f = fopen(fai.c_str(), "r");
    if (!f) return clair_host_fail("%s: cannot open", fai.c_str());
    char line[4096];
    bool found = false;
    long long length = 0, offset = 0, line_bases = 0, line_width = 0;
    while (fgets(line, sizeof line, f)) {
        char *tab = strchr(line, '\t');
        if (!tab) continue;
        *tab = 0;
        if (strcmp(line, ctg)) continue;
        found = sscanf(tab + 1, "%lld\t%lld\t%lld\t%lld", &length, &offset, &line_bases, &line_width) == 4;
        break;
    }
    fclose(f);
    if (!found) return clair_host_fail("%s: contig %s is not in the index", fai.c_str(), ctg);
    if (line_bases <= 0 || line_width < line_bases) return clair_host_fail("%s: bad line lengths for %s", fai.c_str(), ctg);
    int64_t beg0 = 0, end0 = length;                             // samtools faidx: the region clamped to the contig
    if (beg1 >= 0 && end1 >= 0) { beg0 = std::max<int64_t>(beg1, 1) - 1; end0 = std::min<int64_t>(end1, length); }
    const int64_t n = end0 > beg0 ? end0 - beg0 : 0;
    *len = n;
    if (!out) return 0;
    if (cap < n) return clair_host_fail("faidx: %lld bytes do not fit in %lld", (long long)n, (long long)cap);
    if (!n) return 0;
    FILE *fa = fopen(fasta, "rb");
    if (!fa) return clair_host_fail("%s: cannot open", fasta);
    const int64_t first = offset + beg0 / line_bases * line_width + beg0 % line_bases;
    const int64_t last = offset + (end0 - 1) / line_bases * line_width + (end0 - 1) % line_bases;
    std::vector<char> raw((size_t)(last - first + 1));
    const bool ok = fseeko(fa, (off_t)first, SEEK_SET) == 0 && fread(raw.data(), 1, raw.size(), fa) == raw.size();
    fclose(fa);
    if (!ok) return clair_host_fail("%s: truncated at contig %s", fasta, ctg);
    int64_t w = 0;
    for (char c : raw)
        if (c != '\n' && c != '\r' && w < n) out[w++] = c;
    if (w != n) return clair_host_fail("%s: contig %s is shorter than its index says", fasta, ctg);
    return 0;
}

}  // extern "C"
