// compare_vcf's host twin (clair_amd/hostsrc/host_compare.cpp over csrc/compare_core.h) as a stand-alone program, for a build with
// -fsanitize=address,undefined (tests/test_left_align.py): parse -> left_align -> sort if needed -> run on the files it is given.
//
//     left_align_sanitize calls.vcf truth.vcf reference.tsv        reference.tsv: one line `name<TAB>sequence` per contig of the table, in order;
//                                                                  an empty sequence: none loaded
// Prints, per side, the eight statistics of _left_align and the arena, then counts[side][type][outcome] -- what the test compares with the
// library's own answer.  The buffers handed over are exactly as long as their contents, so a read past an end is seen.
#include "../include/clair_host.h"
#include "../clair_amd/csrc/compare_core.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

int clair_host_fail(const char *fmt, ...) {      // host_io.cpp's, without the rest of that file
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return 1;
}

static std::vector<uint8_t> exact(const std::string &s) { return std::vector<uint8_t>(s.begin(), s.end()); }

static std::string slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

#define MUST(call) do { if ((call) != 0) { fprintf(stderr, "failed: %s\n", #call); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc != 4) return clair_host_fail("usage: %s calls.vcf truth.vcf reference.tsv", argv[0]);
    std::vector<uint8_t> text[2] = {exact(slurp(argv[1])), exact(slurp(argv[2]))};
    std::string names, seq;
    std::vector<int64_t> name_off{0}, seq_off{0};
    {
        std::istringstream lines(slurp(argv[3]));
        for (std::string line; std::getline(lines, line);) {
            const size_t tab = line.find('\t');
            if (tab == std::string::npos) return clair_host_fail("reference.tsv: a line without a tab");
            names += line.substr(0, tab);
            seq += line.substr(tab + 1);
            name_off.push_back((int64_t)names.size());
            seq_off.push_back((int64_t)seq.size());
        }
    }
    const std::vector<uint8_t> name_bytes = exact(names), seq_bytes = exact(seq);
    const int n_contigs = (int)name_off.size() - 1;
    clair_host_compare_t *h = nullptr;
    MUST(clair_host_compare_create(&h));
    MUST(clair_host_compare_set_contigs(h, name_bytes.data(), name_off.data(), n_contigs));
    MUST(clair_host_compare_set_regions(h, nullptr, nullptr, nullptr, -1));
    MUST(clair_host_compare_set_reference(h, seq_bytes.data(), seq_off.data(), n_contigs));
    for (int side = 0; side < 2; ++side) {
        int64_t stats[8];
        MUST(clair_host_compare_parse(h, side, text[side].data(), (int64_t)text[side].size(), stats));
        const int64_t n = stats[2];
        MUST(clair_host_compare_left_align(h, side, stats));
        printf("left_align %d:", side);
        for (int k = 0; k < 8; ++k) printf(" %lld", (long long)stats[k]);
        std::vector<uint8_t> arena((size_t)stats[CLAIR_CMP_LA_ARENA]);
        MUST(clair_host_compare_allele_text(h, side, arena.data()));
        printf(" %s\n", std::string(arena.begin(), arena.end()).c_str());
        if (!stats[CLAIR_CMP_LA_SORTED]) {
            std::vector<int64_t> keys((size_t)n), perm((size_t)n);
            MUST(clair_host_compare_keys(h, side, keys.data()));
            std::iota(perm.begin(), perm.end(), (int64_t)0);
            std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return keys[(size_t)a] < keys[(size_t)b]; });
            MUST(clair_host_compare_permute(h, side, perm.data()));
        }
    }
    MUST(clair_host_compare_run(h));
    std::vector<int64_t> counts(CLAIR_CMP_COUNTS);
    MUST(clair_host_compare_counts(h, counts.data()));
    printf("counts:");
    for (int k = 0; k < CLAIR_CMP_AT_HIST; ++k) printf(" %lld", (long long)counts[(size_t)k]);
    printf("\n");
    clair_host_compare_destroy(h);
    return 0;
}
