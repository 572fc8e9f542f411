"""The inflate (inflate.hip) past the cap of its grid, against zlib byte for byte.  k_inflate has one workgroup per member up to
kInflateBlocksMax; beyond that the workgroups stride, and member m + cap is decoded by the workgroup that decoded member m, with
the Huffman tables and s_lens of that member still in LDS.  The largest call of test_gpu_inflate.py has about 4 500 members; the
input here (grid_caps_inputs.i1) has cap + 700 in one piece, which is one launch:

  - the kind of member m (stored at level 0, fixed codes with Z_FIXED, dynamic at level 9) differs from that of member m + cap, and
    the 700 workgroups that take two trips see the six ordered pairs of kinds;
  - a fixed-code member follows a dynamic one whose literal code has all fifteen lengths, a dynamic one follows a stored one;
  - members cap - 1 and cap are empty.

Then the same stream with one member of the second trip damaged, by a wrong CRC or by deflate data cut in half (two of
test_gpu_inflate.py's malformed members): the call is refused with that member's offset and reason, and the context goes on to
inflate the good stream.

Nothing here was tried against planted faults.  A workgroup that took the first trip's member again, or decoded with the tables of
the member before, writes other bytes than zlib's or fails the member's CRC."""
import re

import pytest

import grid_caps_inputs as G
import pbsim3_amd as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(), 0) as c:
        yield c


def inflated(ctx, s):
    got = ctx.inflate_buffer(s.z)
    assert len(got) == len(s.want)
    if got != s.want:
        at = next(i for i, (a, b) in enumerate(zip(got, s.want)) if a != b)
        ends, m = 0, 0
        while ends + len(s.texts[m]) <= at:
            ends, m = ends + len(s.texts[m]), m + 1
        raise AssertionError("byte %d, in member %d (%s)" % (at, m, G.KINDS[G.block_kind(s.cdata[m])]))


def test_i1_members_past_the_workgroups(ctx, capfd, monkeypatch):
    s = G.i1()
    assert P.inflate_bound(s.z) == len(s.want) and s.members > G.MEMBER_CAP
    assert max(sum(len(c) for c in s.cdata), len(s.want)) < G.default_piece_bytes()      # the piece rule: one piece
    monkeypatch.setenv("PBSIM_INFLATE_TRACE", "1")
    capfd.readouterr()
    inflated(ctx, s)
    err = capfd.readouterr().err
    print(err.strip())
    assert re.findall(r"\[inflate\] (\d+) members, (\d+) pieces", err) == [(str(s.members), "1")], err[-2000:]


@pytest.mark.parametrize("damage", sorted(G.DAMAGE))
def test_i2_one_damaged_member_on_the_second_trip(ctx, damage):
    s = G.i1()
    z, m, reason = G.i2(damage)
    assert m >= G.MEMBER_CAP and P.inflate_bound(z) == len(s.want)
    with pytest.raises(P.PbsimError, match="gzip member at byte offset %d: .*%s" % (s.offsets[m], reason)):
        ctx.inflate_buffer(z)
    inflated(ctx, s)
