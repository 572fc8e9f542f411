"""The BGZF member index of the GPU inflate (pbsim_inflate_bound, pbsim3_amd/csrc/inflate_host.cpp) needs no device:
it reads member headers and trailers only.  And pbsim_inflate_buffer refuses a tables-only context."""
import os
import struct

import pytest

import bgzf_writer as W
import pbsim3_amd as P


def data(n, seed=1):
    return bytes((i * 2654435761 + seed) >> 7 & 0xff for i in range(n))


def test_bound_of_bgzip_blocks():
    d = data(3 * W.BGZIP_BLOCK + 1234)
    assert P.inflate_bound(W.bgzf(d)) == len(d)
    assert P.inflate_bound(W.bgzf(d, eof=False)) == len(d)


def test_bound_of_full_64k_members():
    d = bytes(b"ACGT"[x & 3] for x in os.urandom(3 * 65536 + 17))
    z = W.bgzf(d, block=65536)            # ISIZE of exactly 64 KiB, the largest there is
    assert P.inflate_bound(z) == len(d)


def test_bound_of_eof_marker_alone():
    assert P.inflate_bound(W.EOF_MARKER) == 0
    assert P.inflate_bound(b"") == 0


def test_bound_with_other_subfields_first():
    d = data(5000)
    z = W.bgzf(d, block=1000, extra_before=b"XY\x03\x00abc" + b"ZZ\x00\x00")
    assert P.inflate_bound(z) == len(d)


def test_bound_refuses_plain_gzip():
    d = data(100000)
    assert P.inflate_bound(W.plain_gzip(d)) == -1
    assert P.inflate_bound(W.plain_gzip(d[:500]) + W.plain_gzip(d[500:])) == -1
    assert P.inflate_bound(W.bgzf(d) + W.plain_gzip(d)) == -1


def test_bound_refuses_broken_framing():
    d = data(200000)
    z = W.bgzf(d, eof=False)
    assert P.inflate_bound(z[:-1]) == -1                      # truncated last member
    last = z.rfind(b"\x1f\x8b\x08\x04")
    bad = bytearray(z)
    struct.pack_into("<H", bad, last + 16, struct.unpack_from("<H", z, last + 16)[0] + 1)
    assert P.inflate_bound(bytes(bad)) == -1                 # BSIZE past the end
    over = W.member(b"x" * 10, isize=65537)
    assert P.inflate_bound(over) == -1                       # ISIZE over 64 KiB
    assert P.inflate_bound(W.member(b"x" * 10, isize=65536)) == 65536
    bad = bytearray(z)
    bad[last + 12:last + 14] = b"BD"                          # no 'BC' subfield
    assert P.inflate_bound(bytes(bad)) == -1


def test_inflate_buffer_refuses_without_device():
    with P.Context(P.default_params(), -1) as c:
        with pytest.raises(P.PbsimError, match="no HIP device"):
            c.inflate_buffer(W.bgzf(b"ACGT" * 1000))
        with pytest.raises(P.PbsimError, match="not BGZF"):       # other gzip: refused before any device question
            c.inflate_buffer(W.plain_gzip(b"ACGT" * 1000))
