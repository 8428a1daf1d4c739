"""SAM text -> BAM + .bai + the canonical text `samtools view` prints for that BAM (test support, not a test).

Written with Python's zlib and struct only, independently of clair_amd/hostsrc/host_bam.cpp, so that the native reader is checked against
the format and not against itself:
  - BGZF blocks of a configurable size (records straddle blocks), or one record per block; the 28-byte EOF block (optional);
  - records encoded as the SAM spec and htslib's sam_parse1 encode them: SEQ through the nt16 table (lower case -> upper, anything that is
    not an IUPAC code -> N), QUAL '*' -> 0xff, the tags i / A / Z / B:I kept, a CIGAR of more than 65 535 operations stored as the
    <l_seq>S<ref_len>N placeholder with the real one in CG:B:I;
  - a .bai with htslib's bins (reg2bin), per-bin chunks and the 16 kb linear index;
  - canonical(): the 11 mandatory columns samtools prints for the encoded records -- the yardstick, not the source SAM.
"""
import re
import struct
import zlib

NT16 = "=ACMGRSVTWYHKDBN"
_CODE = {c: i for i, c in enumerate(NT16)}
_CODE.update({c.lower(): i for c, i in list(_CODE.items()) if c != "="})
_CODE.update({"U": 8, "u": 8})
CIGAR_OPS = "MIDNSHP=XB"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def nt16(base):
    return _CODE.get(base, 15)


def parse_cigar(text):
    if text == "*":
        return []
    return [(int(n), CIGAR_OPS.index(op)) for n, op in re.findall(r"(\d+)([MIDNSHP=XB])", text)]


def ref_span(ops):
    return sum(n for n, op in ops if op in (0, 2, 3, 7, 8))


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


class Record(object):
    def __init__(self, line, tid_of):
        col = line.rstrip("\n").split("\t")
        self.qname, self.flag = col[0], int(col[1])
        self.tid = -1 if col[2] == "*" else tid_of[col[2]]
        self.pos = int(col[3]) - 1
        self.mapq = int(col[4])
        self.cigar = parse_cigar(col[5])
        self.next_tid = -1 if col[6] == "*" else (self.tid if col[6] == "=" else tid_of[col[6]])
        self.next_pos, self.tlen = int(col[7]) - 1, int(col[8])
        seq = "" if col[9] == "*" else col[9]
        self.seq = [nt16(c) for c in seq]
        self.qual = None if col[10] == "*" or not seq else bytes(ord(c) - 33 for c in col[10])
        self.tags = col[11:]
        self.raw_aux = b""                                  # bytes a test appends behind the encoded tags, as they are

    def end(self):
        """bam_endpos"""
        span = 0 if self.flag & 4 else ref_span(self.cigar)
        return self.pos + max(span, 1)

    def encode(self):
        name = self.qname.encode() + b"\0"
        cigar, aux = self.cigar, b""
        if len(cigar) > 65535:                              # the placeholder and the real CIGAR in CG:B:I (htslib)
            aux += b"CGBI" + struct.pack("<I", len(cigar)) + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar)
            cigar = [(len(self.seq), 4), (ref_span(self.cigar), 3)]
        for t in self.tags:
            tag, typ, val = t.split(":", 2)
            if typ == "i":
                aux += tag.encode() + b"i" + struct.pack("<i", int(val))
            elif typ == "A":
                aux += tag.encode() + b"A" + val.encode()
            elif typ == "Z":
                aux += tag.encode() + b"Z" + val.encode() + b"\0"
            elif typ == "B" and val.startswith("I"):
                v = [int(x) for x in val.split(",")[1:]]
                aux += tag.encode() + b"BI" + struct.pack("<I", len(v)) + struct.pack("<%dI" % len(v), *v)
        seq = bytes((self.seq[i] << 4) | (self.seq[i + 1] if i + 1 < len(self.seq) else 0) for i in range(0, len(self.seq), 2))
        qual = self.qual if self.qual is not None else b"\xff" * len(self.seq)
        body = struct.pack("<iiBBHHHiiii", self.tid, self.pos, len(name), self.mapq, reg2bin(max(self.pos, 0), self.end()) if self.tid >= 0 else 4680,
                           len(cigar), self.flag, len(self.seq), self.next_tid, self.next_pos, self.tlen)
        body += name + b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar) + seq + qual + aux + self.raw_aux
        return struct.pack("<I", len(body)) + body

    def canonical(self, names):
        """the line `samtools view` prints, mandatory columns only"""
        cig = "".join("%d%s" % (n, CIGAR_OPS[op]) for n, op in self.cigar) or "*"
        rnext = "*" if self.next_tid < 0 else ("=" if self.next_tid == self.tid else names[self.next_tid])
        seq = "".join(NT16[c] for c in self.seq) or "*"
        qual = "*" if self.qual is None else "".join(chr(q + 33) for q in self.qual)
        return "\t".join([self.qname, str(self.flag), "*" if self.tid < 0 else names[self.tid], str(self.pos + 1), str(self.mapq), cig, rnext,
                          str(self.next_pos + 1), str(self.tlen), seq, qual]) + "\n"


class Bam(object):
    """bam = Bam(sam_text, refs=[(name, length), ...]); bam.write(path, block=..., per_record=False, index=True, eof=True);
    bam.canonical(); bam.records"""

    def __init__(self, sam_text, refs, sort=True):
        self.refs = list(refs)
        for line in sam_text.splitlines():                  # names a line uses that the caller did not list: references of their own
            col = line.split("\t")
            if line and not line.startswith("@"):
                for name in (col[2], col[6]):
                    if name not in ("*", "=") and name not in [n for n, _ in self.refs]:
                        self.refs.append((name, 1 << 28))
        self.names = [n for n, _ in self.refs]
        tid_of = {n: i for i, n in enumerate(self.names)}
        self.records = [Record(l, tid_of) for l in sam_text.splitlines() if l and not l.startswith("@")]
        if sort:
            self.records.sort(key=lambda r: (r.tid if r.tid >= 0 else 1 << 31, r.pos))

    def header(self):
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in self.refs)
        out = b"BAM\1" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<i", len(self.refs))
        for name, length in self.refs:
            out += struct.pack("<I", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", length)
        return out

    def canonical(self):
        return "".join(r.canonical(self.names) for r in self.records)

    def write(self, path, block=65280, per_record=False, index=True, eof=True):
        """-> bytes written.  block: uncompressed bytes per BGZF block (records straddle blocks); per_record: one record per block."""
        pieces = [self.header()] + [r.encode() for r in self.records]
        stream = b"".join(pieces)
        starts, at = [], len(pieces[0])
        for p in pieces[1:]:
            starts.append(at)
            at += len(p)
        if per_record:
            cuts = [0] + [s for s in starts] + [len(stream)]
        else:
            cuts = list(range(0, len(stream), block)) + [len(stream)]
        cuts = sorted(set(cuts))
        cuts = sorted(set(cuts + [c for a, b in zip(cuts[:-1], cuts[1:]) for c in range(a, b, 65280)]))   # no block holds more than 64 KB
        out, block_at = bytearray(), []                      # block_at: (uncompressed start, compressed offset)
        for a, b in zip(cuts[:-1], cuts[1:]):
            data = stream[a:b]
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            z = c.compress(data) + c.flush()
            block_at.append((a, len(out)))
            out += struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(z) + 25) + z
            out += struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))
        end_coffset = len(out)
        if eof:
            out += EOF_BLOCK
        with open(path, "wb") as f:
            f.write(bytes(out))

        def voff(u):
            if u >= len(stream):
                return end_coffset << 16
            k = max(i for i, (s, _) in enumerate(block_at) if s <= u)
            return block_at[k][1] << 16 | (u - block_at[k][0])
        if index:
            self._write_bai(path + ".bai", [(voff(s), voff(s + len(p))) for s, p in zip(starts, pieces[1:])])
        return len(out)

    def _write_bai(self, path, voffs):
        per_ref = [dict(bins={}, lin={}) for _ in self.refs]
        for r, (beg, end) in zip(self.records, voffs):
            if r.tid < 0:
                continue
            ref = per_ref[r.tid]
            b = reg2bin(max(r.pos, 0), r.end())
            chunks = ref["bins"].setdefault(b, [])
            if chunks and chunks[-1][1] == beg:
                chunks[-1][1] = end
            else:
                chunks.append([beg, end])
            for w in range(max(r.pos, 0) >> 14, ((r.end() - 1) >> 14) + 1):
                ref["lin"].setdefault(w, beg)
        out = b"BAI\1" + struct.pack("<i", len(self.refs))
        for ref in per_ref:
            out += struct.pack("<i", len(ref["bins"]))
            for b in sorted(ref["bins"]):
                out += struct.pack("<Ii", b, len(ref["bins"][b])) + b"".join(struct.pack("<QQ", c[0], c[1]) for c in ref["bins"][b])
            n = max(ref["lin"]) + 1 if ref["lin"] else 0
            lin, last = [], 0
            for w in range(n):
                last = ref["lin"].get(w, last)
                lin.append(last)
            out += struct.pack("<i", n) + b"".join(struct.pack("<Q", v) for v in lin)
        with open(path, "wb") as f:
            f.write(out)


def fasta_of(refs_seq, width=60):
    """{name: seq} -> (fasta text, fai text)"""
    text, fai, at = "", "", 0
    for name, seq in refs_seq.items():
        head = ">%s\n" % name
        body = "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
        fai += "%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), at + len(head), width, width + 1)
        text += head + body
        at += len(head) + len(body)
    return text, fai
