"""A tabix index (.tbi) for a BGZF-compressed VCF, written from the tabix specification (https://samtools.github.io/hts-specs/tabix.pdf).

    records = [(tid, pos, len(ref), start, end), ...]      # file order; start / end: uncompressed offsets of the row and of the byte after it
    write_tbi(path, names, records, writer.virtual_offset)

Layout, all integers little-endian, the whole index BGZF-compressed:
    magic "TBI\\1", n_ref, format = 2 (VCF), col_seq = 1, col_beg = 2, col_end = 0, meta = '#', skip = 0, l_nm, the NUL-terminated names;
    per reference: n_bin, then per bin: bin, n_chunk, (chunk begin, chunk end) virtual offsets; n_intv, the 16 KiB linear index;
    n_no_coor = 0.
A record covers the 0-based half-open interval [POS - 1, POS - 1 + len(REF)); its bin is reg2bin of it; consecutive records of one bin share a
chunk; linear window w holds the virtual offset of the first record that overlaps it, an empty window the value of the window before it
(0 when there is none).  A reference without records has n_bin = 0 and n_intv = 0.  Positions beyond 2^29 need a .csi index, which is out
of scope here as it is for reading.  Reading a .tbi is not part of this module."""
import struct

MAX_POS = 1 << 29
LINEAR_SHIFT = 14


def reg2bin(beg, end):
    """The bin of the 0-based half-open interval [beg, end) (the specification's C function)."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def build_index(n_ref, records):
    """-> per reference (bins {bin: [[start, end], ...]} in uncompressed offsets, linear [start offset or None per window])."""
    refs = [({}, []) for _ in range(n_ref)]
    last = {}                                    # (tid, bin) -> its last chunk, while the records of that bin are consecutive
    previous = None
    for tid, pos, ref_len, start, end in records:
        beg0, end0 = pos - 1, pos - 1 + max(1, ref_len)
        if pos < 1 or end0 > MAX_POS:
            raise ValueError("POS %d (REF of %d bases) is beyond 2^29: that needs a .csi index, which is out of scope (only .tbi is written)" % (pos, ref_len))
        if not 0 <= tid < n_ref:
            raise ValueError("reference index %d outside 0 .. %d" % (tid, n_ref - 1))
        bins, linear = refs[tid]
        key = (tid, reg2bin(beg0, end0))
        if previous == key and last[key][1] == start:
            last[key][1] = end
        else:
            chunk = [start, end]
            bins.setdefault(key[1], []).append(chunk)
            last[key] = chunk
        previous = key
        w1 = (end0 - 1) >> LINEAR_SHIFT
        if len(linear) <= w1:
            linear.extend([None] * (w1 + 1 - len(linear)))
        for w in range(beg0 >> LINEAR_SHIFT, w1 + 1):
            if linear[w] is None or start < linear[w]:
                linear[w] = start
    return refs


def tbi_bytes(names, records, virtual_offset):
    """The uncompressed bytes of the index; virtual_offset maps an uncompressed offset of the data file to coffset << 16 | uoffset."""
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    blob = b"".join(n + b"\0" for n in names)
    out = [b"TBI\1", struct.pack("<8i", len(names), 2, 1, 2, 0, ord("#"), 0, len(blob)), blob]
    for bins, linear in build_index(len(names), records):
        out.append(struct.pack("<i", len(bins)))
        for b in sorted(bins):
            chunks = bins[b]
            out.append(struct.pack("<Ii", b, len(chunks)))
            for start, end in chunks:
                out.append(struct.pack("<QQ", virtual_offset(start), virtual_offset(end)))
        out.append(struct.pack("<i", len(linear)))
        carried = 0
        for start in linear:
            if start is not None:
                carried = virtual_offset(start)
            out.append(struct.pack("<Q", carried))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def write_tbi(path, names, records, virtual_offset, deflate="zlib", device=0, threads=4):
    from clair_amd.bgzf import BgzfWriter
    data = tbi_bytes(names, records, virtual_offset)
    with BgzfWriter(path, deflate=deflate, device=device, threads=threads) as w:
        w.write(data)
    return len(data)
