// What the file drivers of the BAM tools share.  All three (host_bam_index.cpp, host_bam_sort.cpp, host_markdup.cpp): the input as a job --
// the file opened, its header read and checked, where the first record lies -- and the batches of whole BGZF blocks a read of the input is
// made of.  The two that rewrite a BAM (host_bam_sort.cpp, host_markdup.cpp; the job's entry points are host_bam_job.cpp): the twin's output
// stream cut into payloads of 65280 bytes, the payloads handed out, compressed into the blocks of the output and written, the EOF marker
// behind them.  Host only: plain C++17 + zlib.
#pragma once
#include "../../include/clair_host.h"
#include "../csrc/bam_sort_core.h"
#include "bam_header.h"
#include "bgzf_file.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

// the job: clair_host_bam_job_t of include/clair_host.h
struct clair_host_bam_job {
    std::string path;
    FILE *file = nullptr;
    int64_t file_size = 0;
    std::vector<uint8_t> text;                   // the inflated header, and what follows it in its last block
    BamHeader header;
    int64_t coffset = 0, entry = 0;              // where the first record's block starts, the record's offset in it
    ~clair_host_bam_job() { if (file) fclose(file); }
};

namespace clair_job {

using namespace clair_bgzf;
using clair_bsort::PAYLOAD;
using clair_bsort::SLOT;
using Job = ::clair_host_bam_job;

// the BAM header of `path` read and checked into *job (empty); -> 0, or the message set.  kinds: the sentence about files that are no BAM
inline int open_job(const char *path, const char *kinds, Job *job) {
    job->path = path;
    job->file = fopen(path, "rb");
    if (!job->file) return clair_host_fail("%s: cannot open", path);
    if (fseeko(job->file, 0, SEEK_END) != 0) return clair_host_fail("%s: cannot seek", path);
    job->file_size = (int64_t)ftello(job->file);
    uint8_t magic[4] = {0, 0, 0, 0};
    if (job->file_size < BGZF_HEADER || fseeko(job->file, 0, SEEK_SET) != 0 || fread(magic, 1, 4, job->file) != 4 || !gzip_with_extra(magic))
        return clair_host_fail("%s is not a BGZF-compressed BAM %s", path, kinds);
    std::vector<uint8_t> cbuf;
    std::vector<std::pair<int64_t, int64_t>> pieces;          // (position in text, coffset)
    int64_t coffset = 0;
    const auto need = [&](size_t bytes) -> int {
        while (job->text.size() < bytes) {
            if (coffset >= job->file_size) return clair_host_fail("%s: the BAM header is truncated", path);
            cbuf.clear();
            uint32_t csize = 0, isize = 0;
            if (read_block(job->file, path, (uint64_t)job->file_size, (uint64_t)coffset, cbuf, &csize, &isize)) return 1;
            const size_t at = job->text.size();
            job->text.resize(at + isize);
            const int status = inflate_block(cbuf.data(), csize, job->text.data() + at, isize);
            if (status) return clair_host_fail("%s: BGZF block at compressed offset %lld: %s", path, (long long)coffset, inflate_text(status));
            pieces.emplace_back((int64_t)at, coffset);
            coffset += csize;
        }
        return 0;
    };
    if (parse_bam_header(path, "", need, [&] { return (const uint8_t *)job->text.data(); }, &job->header)) return 1;
    const size_t at = job->header.end;
    job->coffset = coffset;
    job->entry = 0;
    if (at < job->text.size()) {                             // the first record: in the last header block, or at the start of the block after it
        size_t k = pieces.size() - 1;
        while (pieces[k].first > (int64_t)at) --k;
        job->coffset = pieces[k].second;
        job->entry = (int64_t)at - pieces[k].first;
    }
    return 0;
}

// one read of the input: up to max_blocks whole blocks a batch, from the first record's block to the end of the file
struct Batches {
    const Job *job;
    int max_blocks;
    int64_t coffset, entry;
    std::vector<uint8_t> cbuf;
    std::vector<int64_t> in_at, offs;
    std::vector<int32_t> csizes, out_lens;
    bool last = false;
    Batches(const Job *j, int blocks) : job(j), max_blocks(blocks), coffset(j->coffset), entry(j->entry) {}
    // the next batch (its record chain starts at `entry`: 0 once a batch went `through`); `last` with the file's last block
    int next() {
        cbuf.clear(); in_at.clear(); offs.clear(); csizes.clear(); out_lens.clear();
        while ((int)offs.size() < max_blocks && coffset < job->file_size) {
            const size_t here = cbuf.size();
            uint32_t csize = 0, isize = 0;
            if (read_block(job->file, job->path.c_str(), (uint64_t)job->file_size, (uint64_t)coffset, cbuf, &csize, &isize)) return 1;
            in_at.push_back((int64_t)here);
            offs.push_back(coffset);
            csizes.push_back((int32_t)csize);
            out_lens.push_back((int32_t)isize);
            coffset += csize;
        }
        last = coffset >= job->file_size;
        return 0;
    }
    // the batch through a backend's entry point (batch, mark), `more` behind the arguments every one of them takes; then on to the next batch
    template <class Fn, class... More> int through(Fn fn, void *ctx, More... more) {
        const int rc = fn(ctx, cbuf.data(), (int64_t)cbuf.size(), (int)offs.size(), in_at.data(), csizes.data(), out_lens.data(), offs.data(), coffset, entry,
                          last ? 1 : 0, more...);
        entry = 0;
        return rc;
    }
};

// payload i of n: in_len[i] bytes at data + i * PAYLOAD -> one BGZF block in its slot, its size in sizes[i]; thread t takes t, t + nt, ...
inline int deflate_payloads(int threads, const uint8_t *data, int n, const int32_t *in_len, uint8_t *out, int32_t *sizes) {
    std::vector<int> rc((size_t)n, 0);
    const auto one = [&](int i) {
        int64_t n_out = 0;
        rc[(size_t)i] = clair_host_deflate_bgzf(data + (int64_t)i * PAYLOAD, in_len[i], out + (int64_t)i * SLOT, &n_out);
        sizes[i] = (int32_t)n_out;
    };
    const int nt = std::max(1, std::min(threads, n));
    if (nt == 1) {
        for (int i = 0; i < n; ++i) one(i);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; ++t) pool.emplace_back([&, t] { for (int i = t; i < n; i += nt) one(i); });
        for (auto &th : pool) th.join();
    }
    for (int i = 0; i < n; ++i) if (rc[(size_t)i]) return clair_host_fail("deflate of payload %d failed", i);
    return 0;
}

// one BGZF block by zlib at level 6; stored when that is what fits the 64 KiB (clair_amd/bgzf.py: zlib_block)
inline int zlib_payload(const uint8_t *data, int32_t len, uint8_t *out, int32_t *size) {
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int level : {6, 0}) {
        z_stream z{};
        if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return clair_host_fail("deflateInit2 failed");
        z.next_in = const_cast<uint8_t *>(data);
        z.avail_in = (uInt)len;
        z.next_out = out + BGZF_HEADER;
        z.avail_out = (uInt)(SLOT - BGZF_HEADER - BGZF_FOOTER);
        const int rc = deflate(&z, Z_FINISH);
        const size_t got = z.total_out;
        deflateEnd(&z);
        if (rc != Z_STREAM_END) continue;
        memcpy(out, head, 16);
        const uint32_t total = (uint32_t)got + BGZF_HEADER + BGZF_FOOTER, crc = (uint32_t)crc32(0L, data, (uInt)len);
        out[16] = (uint8_t)((total - 1) & 0xff);
        out[17] = (uint8_t)((total - 1) >> 8);
        uint8_t *foot = out + BGZF_HEADER + got;
        for (int k = 0; k < 4; ++k) { foot[k] = (uint8_t)(crc >> (8 * k)); foot[4 + k] = (uint8_t)((uint32_t)len >> (8 * k)); }
        *size = (int32_t)total;
        return 0;
    }
    return clair_host_fail("a payload of %d bytes does not fit a BGZF block", len);
}

// n payloads through the compressor the caller chose and into the file.  deflate 0: `slots` holds the blocks already; 1: zlib; 2: the host
// twin of the device compressor on `threads` threads, both over the packed bytes in `raw`.  sizes: in, the payloads' (0: the blocks') sizes
inline int write_payloads(FILE *out, const char *path, const char *out_path, int deflate, int threads, int n, const uint8_t *raw, uint8_t *slots, int32_t *sizes,
                          int64_t *written) {
    if (deflate == 2) {
        const std::vector<int32_t> in_len(sizes, sizes + n);
        if (deflate_payloads(threads, raw, n, in_len.data(), slots, sizes)) return 1;
    } else if (deflate == 1) {
        for (int i = 0; i < n; ++i)
            if (zlib_payload(raw + (int64_t)i * PAYLOAD, sizes[i], slots + (int64_t)i * SLOT, &sizes[i])) return 1;
    }
    for (int i = 0; i < n; ++i) {
        const int32_t cs = sizes[i];
        if (cs < BGZF_HEADER + BGZF_FOOTER || cs > SLOT) return clair_host_fail("%s: a compressed block of %d bytes", path, cs);
        if (fwrite(slots + (int64_t)i * SLOT, 1, (size_t)cs, out) != (size_t)cs) return clair_host_fail("%s: write failed", out_path);
        *written += cs;
    }
    return 0;
}

// ---- the output of a twin: the bytes it has for the file, cut into payloads; what no whole payload takes waits for the next bytes
struct OutStream {
    std::vector<uint8_t> bytes, carry;
    int64_t total = 0;
    void rewind() { carry.clear(); total = 0; }              // a new file
    void begin() { bytes.assign(carry.begin(), carry.end()); }                        // new bytes go behind what was carried over
    // -> the payloads ready (with `last` the partial one too); the rest is carried
    int64_t cut(bool last) {
        total = (int64_t)bytes.size();
        const int64_t payloads = clair_bsort::payloads_of(total, last);
        carry.assign(bytes.begin() + (ptrdiff_t)std::min(total, payloads * PAYLOAD), bytes.end());
        return payloads;
    }
};

// payloads [first, first + n) of the `total` bytes at data -> out: packed as they are, or (compressed) a BGZF block each in its slot; sizes [n]
inline int emit_payloads(const uint8_t *data, int64_t total, int threads, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes, const char *who) {
    if (!out || !sizes || first < 0 || n < 0) return clair_host_fail("%s emit: bad arguments", who);
    if ((first + n - 1) * PAYLOAD >= total && n > 0) return clair_host_fail("%s emit: payloads [%lld, +%d) of %lld bytes", who, (long long)first, n, (long long)total);
    for (int i = 0; i < n; ++i) sizes[i] = (int32_t)std::min(PAYLOAD, total - (first + i) * PAYLOAD);
    data += first * PAYLOAD;
    if (!compressed) {
        if (n) memcpy(out, data, (size_t)((int64_t)(n - 1) * PAYLOAD + sizes[n - 1]));
        return 0;
    }
    const std::vector<int32_t> in_len(sizes, sizes + n);
    return deflate_payloads(threads, data, n, in_len.data(), out, sizes);
}

// ---- the output file of a driver: it holds the header's blocks already; the payloads a backend has ready are appended EMIT at a time
// through the compressor the caller chose (write_payloads), the EOF marker behind the last
struct Writer {
    static constexpr int EMIT = 64;                          // payloads per emit
    const char *path = nullptr, *out_path = nullptr;         // the input (it names the messages about blocks), the output
    int deflate = 0, threads = 1;
    FILE *file = nullptr;
    int64_t written = 0;
    std::vector<uint8_t> slots, raw;
    std::vector<int32_t> sizes;
    ~Writer() { if (file) fclose(file); }
    int open(const char *in_path, const char *to, int deflate_mode, int n_threads) {
        path = in_path; out_path = to; deflate = deflate_mode; threads = n_threads;
        file = fopen(out_path, "ab");
        if (!file) return clair_host_fail("%s: cannot write", out_path);
        slots.resize((size_t)EMIT * SLOT);
        raw.resize(deflate ? (size_t)EMIT * PAYLOAD : 1);
        sizes.resize((size_t)EMIT);
        return 0;
    }
    // emit: the backend's, with its handle; failed(): the driver's message from the backend's, -> nonzero
    template <class Emit, class Failed> int payloads(int64_t n_payloads, Emit emit, void *ctx, Failed failed) {
        for (int64_t at = 0; at < n_payloads; at += EMIT) {
            const int n = (int)std::min<int64_t>(EMIT, n_payloads - at);
            if (emit(ctx, at, n, deflate == 0 ? 1 : 0, deflate == 0 ? slots.data() : raw.data(), sizes.data())) return failed();
            if (write_payloads(file, path, out_path, deflate, threads, n, raw.data(), slots.data(), sizes.data(), &written)) return 1;
        }
        return 0;
    }
    int finish() {
        if (fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, file) != sizeof BGZF_EOF) return clair_host_fail("%s: write failed", out_path);
        written += (int64_t)sizeof BGZF_EOF;
        FILE *f = file;
        file = nullptr;
        if (fclose(f) != 0) return clair_host_fail("%s: write failed", out_path);
        return 0;
    }
};

}  // namespace clair_job
