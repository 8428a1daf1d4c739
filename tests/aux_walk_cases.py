"""Ten hand-encoded BAM records whose stored CIGAR is the <l_seq>S<ref_len>N placeholder, one per branch of the walk over the aux fields that
looks for the real CIGAR in CG:B:I (test support, not a test), and that walk written out from the SAM specification (4.2.4) and htslib's
bam_tag2cigar, independently of csrc/bam_record_core.h.  Used on the CPU (test_bam_reader.py) and on the device (test_bam_gpu.py)."""
import struct

import bam_fixture as bf

CTG, REF_LEN = "chrA", 400
REAL = [(4, 0), (1, 1), (5, 0)]                             # 4M1I5M: 10 bases of the read, 9 of the reference
PLACEHOLDER = "10S9N"
SEQ = "ACGTACGTAC"
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def _ops(ops):
    return b"".join(struct.pack("<I", n << 4 | op) for n, op in ops)


def _cg(sub=b"I", ops=REAL):
    return b"CGB" + sub + struct.pack("<I", len(ops)) + _ops(ops)


# (name, aux bytes): the placeholder stands unless the rule below finds the real CIGAR
CASES = [
    ("cg_first", _cg() + b"NMi" + struct.pack("<i", 3)),
    ("cg_after_i_Z_BS", b"NMi" + struct.pack("<i", 3) + b"RGZgroup1\0" + b"XSBS" + struct.pack("<IHHH", 3, 7, 8, 9) + _cg()),
    ("cg_signed_subtype", b"XAAq" + _cg(b"i")),
    ("cg_subtype_S", b"CGBS" + struct.pack("<IHHH", 3, 64, 17, 80) + _cg()),
    ("cg_type_Z", b"CGZ4M1I5M\0" + _cg()),
    ("cg_count_below_n_cigar", b"CGBI" + struct.pack("<I", 1) + _ops([(10, 0)])),
    ("Z_without_nul", b"NMi" + struct.pack("<i", 3) + b"XZZnever ends"),
    ("B_count_past_the_end", b"XBBI" + struct.pack("<I", 1000) + bytes(8)),
    ("unknown_type_before_cg", b"XQ?\0\0" + _cg()),
    ("two_byte_tail", b"NMi" + struct.pack("<i", 3) + b"CG"),
]


def real_cigar(aux, n_cigar):
    """the operations of CG:B:I (or B:i) when the first CG tag is one with at least n_cigar of them; None when the stored CIGAR stands:
    another CG, or a tag before it that cannot be stepped over"""
    at = 0
    while at + 3 <= len(aux):
        tag, typ, v = aux[at:at + 2], chr(aux[at + 2]), at + 3
        if typ in FIXED:
            size = FIXED[typ]
        elif typ in "ZH":
            nul = aux.find(b"\0", v)
            if nul < 0:
                return None
            size = nul - v + 1
        elif typ == "B":
            if v + 5 > len(aux):
                return None
            sub, count = chr(aux[v]), struct.unpack_from("<I", aux, v + 1)[0]
            if sub not in "cCsSiIf" or count * FIXED[sub] > len(aux) - v - 5:
                return None
            if tag == b"CG":
                if sub not in "iI" or count < n_cigar or count >= 1 << 29:
                    return None
                return [(c >> 4, c & 15) for c in struct.unpack_from("<%dI" % count, aux, v + 5)]
            size = 5 + count * FIXED[sub]
        else:
            return None
        if tag == b"CG":
            return None
        at = v + size
    return None


def expected_cigar(aux):
    ops = real_cigar(aux, 2)
    return PLACEHOLDER if ops is None else "".join("%d%s" % (n, bf.CIGAR_OPS[op]) for n, op in ops)


def bam():
    """-> (bf.Bam of the ten records in CASES' order, [expected CIGAR column]).  Every record is 1 (mod 4) bytes long, by its read name, so
    that consecutive records start at offsets 0, 1, 2, 3 (mod 4) of the chunk they are read into."""
    lines = ["%s\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*" % (name, CTG, 20 + 10 * k, PLACEHOLDER, SEQ) for k, (name, _) in enumerate(CASES)]
    out = bf.Bam("\n".join(lines) + "\n", [(CTG, REF_LEN)])
    for rec, (_, aux) in zip(out.records, CASES):
        rec.raw_aux = aux
        while len(rec.encode()) % 4 != 1:
            rec.qname += "x"
    return out, [expected_cigar(aux) for _, aux in CASES]
