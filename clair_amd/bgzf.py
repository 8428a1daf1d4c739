"""BgzfWriter: a BGZF file (the blocked gzip of samtools / htslib / bgzip) written block by block.

    w = BgzfWriter("calls.vcf.gz", deflate="host", threads=4)       # or an open binary file object
    w.write(data); ...; w.close()
    w.virtual_offset(uncompressed_offset)                           # after close(): coffset << 16 | uoffset, for an index

The stream is cut every 65280 bytes, line ends or not, as bgzip cuts it; close() appends the 28-byte EOF marker.  Who compresses a block:
  zlib     Python's zlib at level 6 (always there);
  host     the host twin of the device compressor (clair_host_deflate_bgzf), `threads` blocks side by side;
  device   the GPU, a wave per block (clair_deflate_blocks; csrc/deflate.hip).
`host` and `device` write the same bytes (docs/merge_vcf.md)."""
import struct
import zlib

BLOCK_INPUT = 65280             # bgzip's 0xff00
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BACKENDS = ("zlib", "host", "device")


def zlib_block(data):
    """One BGZF block by zlib level 6; stored when that is what fits the 64 KiB."""
    for level in (6, 0):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        stream = c.compress(data) + c.flush()
        if len(stream) + 26 <= 65536:
            break
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(stream) + 25) + stream
            + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


class BgzfWriter(object):
    def __init__(self, path_or_fileobj, deflate="zlib", device=0, threads=4, batch_blocks=256):
        if deflate not in BACKENDS:
            raise ValueError("deflate %r: one of %s" % (deflate, ", ".join(BACKENDS)))
        if not 1 <= int(threads) <= 64 or not 1 <= int(batch_blocks) <= 16384:
            raise ValueError("threads 1 .. 64, batch_blocks 1 .. 16384")
        self.deflate, self.threads, self.batch_blocks = deflate, int(threads), int(batch_blocks)
        self._own_file = isinstance(path_or_fileobj, (str, bytes))
        self._pool = self._deflater = None
        if deflate == "host":
            from clair_amd import _hostapi
            _hostapi.load()
            if self.threads > 1:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(max_workers=self.threads)
        elif deflate == "device":
            from clair_amd import _capi
            self._deflater = _capi.Deflater(device=int(device), max_blocks=self.batch_blocks)       # EngineError without a GPU: no fallback
        self._f = open(path_or_fileobj, "wb") if self._own_file else path_or_fileobj
        self._pending = bytearray()
        self._in = 0                    # uncompressed bytes taken
        self._out = 0                   # compressed bytes written
        self._starts = []               # per block written: (uncompressed offset, compressed offset)
        self._block_in = 0              # uncompressed offset of the next block to be written
        self.closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def tell(self):
        """The uncompressed offset of the next byte written."""
        return self._in

    def write(self, data):
        if self.closed:
            raise ValueError("write to a closed BgzfWriter")
        self._pending += data
        self._in += len(data)
        whole = len(self._pending) // BLOCK_INPUT
        if whole >= self.batch_blocks:
            self._compress(whole)
        return len(data)

    def _compress(self, n_blocks, tail=False):
        """The first n_blocks whole blocks of the pending bytes (and, with tail, what is left after them) go to the file, in order."""
        buf = bytes(self._pending[:n_blocks * BLOCK_INPUT]) if not tail else bytes(self._pending)
        del self._pending[:len(buf)]
        at = 0
        while at < len(buf):
            batch = buf[at:at + self.batch_blocks * BLOCK_INPUT]
            at += len(batch)
            lens = [min(BLOCK_INPUT, len(batch) - k) for k in range(0, len(batch), BLOCK_INPUT)]
            if self.deflate == "device":
                import numpy as np
                offs = np.arange(len(lens), dtype=np.int64) * BLOCK_INPUT
                out, csize = self._deflater.blocks(batch, offs, np.array(lens, dtype=np.int32))
                blocks = [out[i, :csize[i]].tobytes() for i in range(len(lens))]
            else:
                pieces = [batch[k:k + BLOCK_INPUT] for k in range(0, len(batch), BLOCK_INPUT)]
                if self.deflate == "zlib":
                    blocks = [zlib_block(p) for p in pieces]
                else:
                    from clair_amd._hostapi import deflate_bgzf
                    blocks = list(self._pool.map(deflate_bgzf, pieces)) if self._pool else [deflate_bgzf(p) for p in pieces]
            for n, block in zip(lens, blocks):
                self._starts.append((self._block_in, self._out))
                self._block_in += n
                self._out += len(block)
            self._f.write(b"".join(blocks))

    def flush(self):
        """Every pending byte goes out; the block in progress is ended (as bgzf_flush does)."""
        if self._pending:
            self._compress(0, tail=True)

    def close(self):
        if self.closed:
            return
        self.flush()
        self._f.write(EOF_MARKER)
        self._eof_at = self._out
        self._out += len(EOF_MARKER)
        self.closed = True
        if self._own_file:
            self._f.close()
        else:
            self._f.flush()
        if self._pool:
            self._pool.shutdown()
        if self._deflater:
            self._deflater.close()

    def virtual_offset(self, uncompressed_offset):
        """coffset << 16 | uoffset of an uncompressed offset 0 .. tell().  An offset at a block's end is the next block's start (uoffset 0,
        what bgzf_tell gives after a flush); the end of the data is the start of the EOF block."""
        if not self.closed:
            raise ValueError("virtual_offset: close() the writer first")
        u = int(uncompressed_offset)
        if not 0 <= u <= self._in:
            raise ValueError("offset %d outside the %d bytes written" % (u, self._in))
        if u == self._in:
            return self._eof_at << 16
        import bisect
        k = bisect.bisect_right(self._starts, (u, float("inf"))) - 1
        ustart, cstart = self._starts[k]
        return cstart << 16 | (u - ustart)

    @property
    def compressed_bytes(self):
        return self._out
