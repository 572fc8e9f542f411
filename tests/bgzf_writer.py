"""A test-side BGZF writer (SAMv1 4.1) on zlib: gzip members of at most `block` input bytes, each with the 'BC' extra
subfield that holds the member's size, optionally behind other subfields; plain gzip for the non-BGZF cases."""
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZIP_BLOCK = 65280          # what bgzip puts in one member


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def member(data, cdata=None, extra_before=b"", crc=None, isize=None, **kw):
    """one BGZF member of `data`; cdata/crc/isize override what goes in (malformed members)"""
    if cdata is None:
        cdata = raw_deflate(data, **kw)
    xlen = len(extra_before) + 6
    bsize = 12 + xlen + len(cdata) + 8 - 1
    assert bsize < 65536
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra_before + b"BC\x02\x00" + \
        struct.pack("<H", bsize)
    crc = zlib.crc32(data) & 0xffffffff if crc is None else crc
    isize = len(data) if isize is None else isize
    return head + cdata + struct.pack("<II", crc, isize)


def bgzf(data, block=BGZIP_BLOCK, eof=True, **kw):
    out = [member(data[i:i + block], **kw) for i in range(0, len(data), block)]
    return b"".join(out) + (EOF_MARKER if eof else b"")


def plain_gzip(data, level=6):
    """one ordinary gzip member (no extra field)"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()
