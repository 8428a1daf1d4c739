// Host-side helpers of the Clair hot path (include/clair_host.h): the indel look-up over packed alignments, the twin of the device's
// (clair_amd/csrc/indel_lookup.hip).  Plain C++17, no HIP.  The table itself is csrc/indel_lookup_core.h, the code the device library
// runs too when a query overflows its hit list, so that both answer with the same bytes.
#include "../../include/clair_host.h"
#include "../../include/clair_reads.h"
#include "../csrc/indel_lookup_core.h"

#include <vector>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

extern "C" int clair_host_indel_table(const clair_read_t *const *reads, const int64_t *n_reads, const clair_op_t *const *ops, const int64_t *n_ops,
                                      const uint8_t *const *seq, const int64_t *seq_bytes, int64_t n_slabs, const int64_t *positions, int64_t n,
                                      clair_indel_entry_t *entries, int capacity, int32_t *n_entries, int32_t *depth, uint32_t *status) {
    if (n_slabs < 0 || n < 0 || capacity < 1) return clair_host_fail("indel table: bad sizes");
    if (n_slabs > 0 && (!reads || !n_reads || !ops || !n_ops || !seq || !seq_bytes)) return clair_host_fail("indel table: NULL slab arrays");
    if (n > 0 && (!positions || !entries || !n_entries || !depth || !status)) return clair_host_fail("indel table: NULL query arrays");
    for (int64_t q = 1; q < n; ++q)
        if (positions[q] <= positions[q - 1]) return clair_host_fail("indel table: positions must ascend strictly (entry %lld)", (long long)q);
    std::vector<ClairLookupSlab> slabs((size_t)n_slabs);
    for (int64_t s = 0; s < n_slabs; ++s) {
        if (n_reads[s] < 0 || n_ops[s] < 0 || seq_bytes[s] < 0 || (n_reads[s] > 0 && (!reads[s] || !ops[s])))
            return clair_host_fail("indel table: slab %lld is not a slab", (long long)s);
        slabs[(size_t)s] = ClairLookupSlab{reads[s], n_reads[s], ops[s], n_ops[s], seq[s], seq_bytes[s]};
    }
    clair_indel_table_core(slabs.data(), n_slabs, positions, n, nullptr, entries, capacity, n_entries, depth, status);
    return 0;
}
