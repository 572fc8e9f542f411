"""The prepared reference, base by base, against the plain model (ref_prep_model.py).

launch_prepare_reference (k_hp_breaks, k_hp_carry, k_hp_final) upper-cases a record, gives every base its homopolymer
class, counts the census and puts the class == 11 flag into bit 7 of the sequence bytes or writes the hp array.  The
simulated reads show a wrong class only where a deletion draw falls between two thresholds; here every byte and every
count is read back (pbsim_dump_table 3-6) and compared exactly, at the kernels' three seams: a thread's 16 bytes, a tile
of 4096 bases and the 1024-tile chunks of the scans in k_hp_carry (base 4 194 304).

Every case runs in both modes: FLAG (--hp-del-bias 1, no byte >= 0x80: bit 7 == (class == 11), the hp array refused)
and ARRAY (--hp-del-bias 3 behind add_hp_census / finish_hp_census: hp == class, no bit added, and the accumulated
census equals the sum of the models' over the records added)."""
import ctypes as C

import numpy as np
import pytest

import pbsim3_amd as P
import ref_prep_model as M

pytestmark = pytest.mark.gpu

TILE = 4096                    # kHpTile
CHUNK = 1024 * TILE            # tiles per pass of the one-workgroup scans of k_hp_carry, in bases
BASES = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
FLAG, ARRAY = 1.0, 3.0         # --hp-del-bias of the two modes
MODES = [pytest.param(FLAG, id="flag"), pytest.param(ARRAY, id="array")]


def _rand(rng, n, alphabet=BASES):
    alphabet = np.frombuffer(alphabet, dtype=np.uint8) if isinstance(alphabet, bytes) else alphabet
    return alphabet[rng.integers(0, alphabet.size, n)].tobytes()


def _where(i):
    return f"base {i} (tile {i // TILE}, offset {i % TILE})"


def _same(what, got, want):
    """exact; names the first and the last differing base, each with its tile and its offset within the tile"""
    got = np.frombuffer(got, dtype=np.uint8)
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i, j = int(bad[0]), int(bad[-1])
        pytest.fail(f"{what}: {bad.size} of {want.size} bases differ, the first at {_where(i)}, the last at {_where(j)}: "
                    f"got {int(got[i])}, want {int(want[i])}; bases {max(i - 3, 0)}..{i + 3} got "
                    f"{got[max(i - 3, 0):i + 4].tolist()}, want {want[max(i - 3, 0):i + 4].tolist()}")


def _census(ctx, which):
    return np.frombuffer(ctx.dump_table(which), dtype=np.int64)


def _check_dumps(ctx, what, seq, hp, census, flag):
    """dumps 3 / 4 / 5 of the context's current unit against the model's (seq, hp, census)"""
    _same(f"{what}: sequence bytes", ctx.dump_table(3), seq)
    if flag:
        with pytest.raises(P.PbsimError, match="hp array is not written"):
            ctx.dump_table(4)
    else:
        _same(f"{what}: hp bytes", ctx.dump_table(4), hp)
    assert _census(ctx, 5).tolist() == census.tolist(), (what, "census of the record")


class Wgs:
    """a wgs context of one mode; ARRAY mode adds every record to the census first and keeps the models' sum beside it"""

    def __init__(self, bias):
        self.bias = bias
        self.ctx = P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, hp_del_bias=bias), 0)
        self.total = np.zeros(M.SLOTS, dtype=np.int64)

    def check(self, what, rec, set_reference=None):
        """prepares `rec` (through set_reference(ctx) if given) and compares what comes back; returns whether bit 7 carries the flag"""
        ctx = self.ctx
        flag = M.flag_mode(rec, self.bias)
        seq, hp, census = M.prepare(rec, flag=flag)
        if self.bias != 1:
            ctx.add_hp_census(rec)
            ctx.finish_hp_census()
            self.total += census
            assert _census(ctx, 6).tolist() == self.total.tolist(), (what, "accumulated census")
        if set_reference is None:
            ctx.set_reference(rec, 1)
        else:
            set_reference(ctx)
        _check_dumps(ctx, what, seq, hp, census, flag)
        return flag


@pytest.fixture(scope="module")
def wgs():
    made = {}

    def get(bias):
        if bias not in made:
            made[bias] = Wgs(bias)
        return made[bias]
    yield get
    for w in made.values():
        w.ctx.close()


def _put_run(buf, start, run):
    """writes `run` at `start` and makes the bases on both sides other letters than the run's (and than each other)"""
    letter = bytes(run[:1]).upper()
    others = [c for c in b"ACGT" if c != letter[0]]
    assert start >= 0 and start + len(run) <= len(buf)
    buf[start:start + len(run)] = run
    if start > 0:
        buf[start - 1] = others[0]
    if start + len(run) < len(buf):
        buf[start + len(run)] = others[1]


def _mixed_case(rng, letter, n):
    return bytes(letter[0] + 32 * int(b) for b in rng.integers(0, 2, n))


@pytest.mark.parametrize("bias", MODES)
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 4095, 4096, 4097, 8191, 8193, 65537])
def test_lengths(wgs, bias, n):
    """the partial last thread (the byte-store tail of k_hp_final), the partial last tile, a one-base record"""
    rng = np.random.default_rng(1000 + n)
    wgs(bias).check(f"random record of {n}", _rand(rng, n))


@pytest.mark.parametrize("bias", MODES)
@pytest.mark.parametrize("s", [16, TILE, 2 * TILE])
def test_runs_at_a_seam(wgs, bias, s):
    """runs of r in {2, 10, 11, 12, 13, 22, 23} that end at s - 1, start at s and straddle s (r // 2 bases in front of
    it), other letters on both sides; a run that ends at s - 1 needs r <= s, so r = 22 and 23 have no such case at s = 16"""
    rng = np.random.default_rng(2000 + s)
    w = wgs(bias)
    for r in (2, 10, 11, 12, 13, 22, 23):
        for place, start in (("ends at s - 1", s - r), ("starts at s", s), ("straddles s", s - r // 2)):
            if start < 0:
                continue
            buf = bytearray(_rand(rng, s + TILE + 37))
            letter = b"ACGT"[r % 4:r % 4 + 1]
            _put_run(buf, start, _mixed_case(rng, letter, r))
            rec = bytes(buf)
            hp = M.prepare(rec)[1]
            assert set(hp[start:start + r].tolist()) == {r if r <= 11 else 11 if r & 1 else 10}   # the case is what it says
            w.check(f"run of {r} that {place}, s = {s}", rec)


@pytest.mark.parametrize("bias", MODES)
def test_runs_over_several_tiles(wgs, bias):
    rng = np.random.default_rng(3000)
    w = wgs(bias)
    rec = (_rand(rng, 3000) + b"c" + b"A" * 9001 + b"g" + _rand(rng, 500) + b"t" + b"C" * 12000 + b"G" + b"N" * 10000 +
           b"a" + _rand(rng, 2500))
    hp = M.prepare(rec)[1]
    assert (hp[3001], hp[3001 + 9001 + 502], hp[3001 + 9001 + 502 + 12001]) == (11, 10, 1)
    w.check("9001 A, 12000 C, 10000 N inside random sequence", rec)
    # ONE run: every tile behind the first has no break, carry_next is the record's length
    w.check("3 * 4096 + 5 G", b"G" * (3 * TILE + 5))
    w.check("3 * 4096 + 6 G", b"G" * (3 * TILE + 6))
    w.check("only N", _rand(rng, 2 * TILE + 9, b"Nn"))
    w.check("only N, one letter", b"N" * (TILE + 1))


@pytest.mark.parametrize("bias", MODES)
def test_case_folding(wgs, bias):
    rng = np.random.default_rng(4000)
    w = wgs(bias)
    rec = _rand(rng, 100, b"ACGT") + b"c" + b"aAaAaAaAaAaA" + b"g" + _rand(rng, 100, b"ACGT") + b"c" + b"nNnN" + b"g"
    seq, hp, _ = M.prepare(rec)
    assert hp[101:113].tolist() == [10] * 12 and hp[215:219].tolist() == [1] * 4 and bytes(seq[215:219]) == b"NNNN"
    w.check("aAaAaAaAaAaA is one run of 12, n counts as N", rec)
    # a lower-case run that meets an upper-case run of the same letter across a tile seam: one run of 13
    buf = bytearray(_rand(rng, 2 * TILE + 50))
    _put_run(buf, TILE - 6, b"t" * 6 + b"T" * 7)
    rec = bytes(buf)
    assert M.prepare(rec)[1][TILE - 6:TILE + 7].tolist() == [11] * 13
    w.check("tttttt|TTTTTTT across the tile seam", rec)
    buf = bytearray(_rand(rng, 2 * TILE + 50))
    _put_run(buf, TILE - 7, b"G" * 7 + b"g" * 5)
    w.check("GGGGGGG|ggggg across the tile seam", bytes(buf))


@pytest.mark.parametrize("bias", MODES)
def test_bytes_with_bit_7(wgs, bias):
    """bytes >= 0x80 switch the flag off whatever the bias: the hp array answers, the bytes come back upper-cased with
    their high bits as given"""
    rng = np.random.default_rng(5000)
    w = wgs(bias)
    recs = {"13 x 0xC4": _rand(rng, 1500) + b"\xc4" * 13 + _rand(rng, 300),
            "12 x 0xFF": _rand(rng, 700) + b"\xff" * 12 + _rand(rng, 300),
            "high bytes in random sequence": _rand(rng, TILE + 300, b"ACGTacgtNn\x80\xe9\xc4\xff"),
            "runs, high bytes and hp 11 of an ASCII letter": _rand(rng, 1500) + b"\xc4" * 13 + _rand(rng, 700, b"ACGT\x80\xe9") +
            b"c" + b"A" * 11 + b"g" + _rand(rng, 1500) + b"\xff" * 12 + _rand(rng, 300),
            "one high byte, the record's last, in another tile than an hp 11 run": b"c" + b"A" * 11 + b"g" + _rand(rng, 2 * TILE) + b"\x80"}
    for what, rec in recs.items():
        assert not w.check(what, rec), what
    # an ASCII record behind them: the flag is back (and the refusal with it)
    assert w.check("ASCII again", b"c" + b"A" * 11 + _rand(rng, 200)) == (bias == 1)


def _chunk_seam_records(rng):
    """The records for the seam between the scans' chunks 0 and 1 (tile 1024, base 4 194 304).  A run of 13 across the
    seam and a run of 6001 from base 4 190 000 overlap, so they are two records; a record of 4 194 304 + 4096 + 7 bases
    ends in tile 1025, so the run `over tiles 1020..1027` is there a run from tile 1020 to four bases before the record's
    end, and a longer record holds the run that covers tiles 1020..1027 with more tiles of chunk 1 behind it.

    A carry that is lost shows in a run's class through the PARITY of the wrong run length alone (both are over 11): a
    start taken as base 0 shows only for a run with an odd start, an end taken as the record's length only where the
    length and the true end differ by an odd number.  The records above have even starts and even distances, so each
    has a neighbour of the other parity behind it."""
    n = CHUNK + TILE + 7
    base = np.frombuffer(_rand(rng, CHUNK + 5 * TILE + 7), dtype=np.uint8)
    out = []

    def add(what, length, start, run):
        buf = bytearray(base[:length].tobytes())
        _put_run(buf, start, run)
        out.append((what, bytes(buf), start, len(run), len(run) if len(run) <= 11 else 10 + len(run) % 2))
    t1020 = 1020 * TILE + 5
    add("run of 13 across base 4 194 304", n, CHUNK - 6, b"A" * 13)
    add("6001 T from base 4 190 000 (tiles 1022..1024)", n, 4_190_000, b"T" * 6001)
    add("one run from tile 1020 to four bases before the record's end in tile 1025", n, t1020, b"C" * (n - 4 - t1020))
    add("one run over tiles 1020..1027", CHUNK + 5 * TILE + 7, t1020, b"G" * (1027 * TILE + 4090 - t1020))
    add("run of 12 across base 4 194 304", n, CHUNK - 6, b"A" * 12)
    add("run of 13 across base 4 194 304, odd start", n, CHUNK - 5, b"A" * 13)
    add("6000 T from base 4 190 001", n, 4_190_001, b"T" * 6000)
    add("one run from tile 1020 to three bases before the record's end", n, t1020, b"C" * (n - 3 - t1020))
    return out


@pytest.fixture(scope="module")
def chunk_seam_records():
    return _chunk_seam_records(np.random.default_rng(6000))


@pytest.mark.parametrize("bias", MODES)
@pytest.mark.parametrize("which", range(8))
def test_scan_chunk_seam(wgs, chunk_seam_records, bias, which):
    """k_hp_carry scans 1024 tiles at a time: the carry into chunk 1 is chunk 0's running maximum, the carry into chunk 0
    is chunk 1's running minimum"""
    what, rec, start, r, cls = chunk_seam_records[which]
    hp = M.prepare(rec)[1]
    assert set(hp[start:start + r].tolist()) == {cls} and start < CHUNK < start + r and cls >= 10, what
    wgs(bias).check(what, rec)


UNIT_KINDS = {"trans_errhmm": (P.STRATEGY_TRANS, P.METHOD_ERR, True), "trans_qshmm": (P.STRATEGY_TRANS, P.METHOD_QS, False),
              "templ_errhmm": (P.STRATEGY_TEMPL, P.METHOD_ERR, True), "templ_qshmm": (P.STRATEGY_TEMPL, P.METHOD_QS, True)}


@pytest.mark.parametrize("bias", MODES)
@pytest.mark.parametrize("kind", sorted(UNIT_KINDS))
def test_units(kind, bias):
    """set_transcripts / set_templates: the units with a line feed behind each; the first byte of a unit keeps its case
    except for qshmm transcripts; no run crosses a separator; the census leaves the separators out"""
    strategy, method, keep_first = UNIT_KINDS[kind]
    rng = np.random.default_rng(7000)

    def lens(*ls):
        return [_rand(rng, n) for n in ls]
    sets = {
        "the kept a splits the run": [b"a" + b"A" * 12 + b"c", b"g" + b"G" * 10, b"n" + b"N" * 3, b"t"],
        "a unit ends in the letter the next one starts with": [_rand(rng, 40) + b"c" + b"G" * 6, b"G" * 5 + b"c" + _rand(rng, 30) + b"tg",
                                                                b"gG" + b"a" * 11, b"A" * 2 + b"c"],
        # separators at bases 15, 32, 50 / 16, 34, 50 / 17, 33, 50: the last and the first byte of a thread's 16
        "15 16 17": lens(15, 16, 17), "16 17 15": lens(16, 17, 15), "17 15 16": lens(17, 15, 16),
        # separators at bases 4095 and 8192 / 4096 / 4097 and 8193: the last and the first byte of a tile
        "4095 4096 4097": lens(4095, 4096, 4097), "4096 4097 4095": lens(4096, 4097, 4095), "4097 4095 4096": lens(4097, 4095, 4096),
        "runs up to the separators on both seams": [b"c" + b"T" * 14, b"T" * 16, b"t" * (TILE - 35) + b"c", b"c" * 13, b"C" * (TILE - 14), b"C"],
        "one unit of one base": [b"N"],
    }
    with P.Context(P.default_params(strategy=strategy, method=method, hp_del_bias=bias), 0) as ctx:
        for what, units in sets.items():
            raw = M.concat_units(units)
            flag = M.flag_mode(raw, bias)
            seq, hp, census = M.prepare(raw, units=True, keep_first=keep_first, flag=flag)
            assert census.sum() == sum(len(u) for u in units)
            ids = ["u%d" % i for i in range(len(units))]
            if strategy == P.STRATEGY_TRANS:
                ctx.set_transcripts(ids, [1] * len(units), [0] * len(units), units)
            else:
                ctx.set_templates(ids, units)
            _check_dumps(ctx, f"{kind}, {what}", seq, hp, census, flag)


@pytest.mark.parametrize("bias", MODES)
def test_prefetched_record_is_prepared_like_one_set_directly(wgs, bias):
    """record A current, B prefetched and adopted: the dumps are B's, through device pointers and through host pointers.
    Behind the prefetch the caller's bytes are overwritten with one letter, so only the ADOPTED copy can give B: had
    set_reference* missed the prefetch it would prepare a record of Ts."""
    import torch
    rng = np.random.default_rng(8000)
    a = _rand(rng, 3 * TILE + 11) + b"c" + b"T" * 11 + b"g"
    buf = bytearray(_rand(rng, 2 * TILE + 17))
    _put_run(buf, TILE - 5, b"A" * 13)
    _put_run(buf, 100, b"N" * 12)
    b = bytes(buf)
    w = wgs(bias)
    w.check("A", a)
    w.check("B set directly", b)
    direct = [w.ctx.dump_table(3), None if M.flag_mode(b, bias) else w.ctx.dump_table(4), w.ctx.dump_table(5)]
    ta, tb = (torch.frombuffer(bytearray(r), dtype=torch.uint8).cuda() for r in (a, b))
    torch.cuda.synchronize()

    def by_device(ctx):
        ctx.set_reference_device(ta.data_ptr(), ta.numel(), 1)
        ctx.prefetch_reference_device(tb.data_ptr(), tb.numel())
        P._check(ctx.lib.pbsim_device_synchronize(ctx.h))     # the prefetch has read the tensor
        tb.fill_(ord("T"))
        torch.cuda.synchronize()
        ctx.set_reference_device(tb.data_ptr(), tb.numel(), 2)
    ha, hb = (C.create_string_buffer(r, len(r)) for r in (a, b))

    def by_host(ctx):
        P._check(ctx.lib.pbsim_set_reference(ctx.h, C.cast(ha, C.c_void_p), len(a), 1))
        P._check(ctx.lib.pbsim_prefetch_reference(ctx.h, C.cast(hb, C.c_char_p), len(b)))
        P._check(ctx.lib.pbsim_device_synchronize(ctx.h))     # the prefetch has read the buffer
        C.memset(hb, ord("T"), len(b))
        P._check(ctx.lib.pbsim_set_reference(ctx.h, C.cast(hb, C.c_void_p), len(b), 2))
    for what, how in (("device pointers", by_device), ("host pointers", by_host)):
        w.check(f"B prefetched and adopted, {what}", b, set_reference=how)
        got = [w.ctx.dump_table(3), None if M.flag_mode(b, bias) else w.ctx.dump_table(4), w.ctx.dump_table(5)]
        assert got == direct, what
    assert tb.cpu().numpy().tobytes() == hb.raw[:len(b)] == b"T" * len(b)


@pytest.mark.parametrize("bias", MODES)
def test_the_callers_memory_is_left_alone(wgs, bias):
    """set_reference_device prepares an owned copy: lower case, the flag bit and the rest stay out of the caller's tensor"""
    import torch
    rng = np.random.default_rng(9000)
    rec = _rand(rng, TILE + 100) + b"c" + b"a" * 11 + b"g" + _rand(rng, 50)
    t = torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    w = wgs(bias)
    w.check("record on the device", rec, set_reference=lambda ctx: ctx.set_reference_device(t.data_ptr(), t.numel(), 1))
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == rec
    assert w.ctx.dump_table(3) != rec       # (the prepared bytes do differ: the check above could see a change)


@pytest.mark.parametrize("bias", MODES)
def test_census_is_of_the_last_record_alone(wgs, bias):
    rng = np.random.default_rng(10000)
    w = wgs(bias)
    recs = [_rand(rng, 5000), b"A" * 11 + b"C" * 7 + b"N" * 30 + b"G" * 12, _rand(rng, 300, b"AC")]
    seen = []
    for i, rec in enumerate(recs):
        w.check(f"record {i}", rec)
        seen.append(_census(w.ctx, 5).tolist())
        assert seen[-1] == M.prepare(rec)[2].tolist()
    assert len({tuple(s) for s in seen}) == 3
    assert seen[1] == [0, 30, 0, 0, 0, 0, 0, 7, 0, 0, 12, 11]


def test_nothing_to_dump():
    """no unit prepared yet, or a tables-only context: refused with a message, no stale memory"""
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), 0) as ctx:
        for which in (3, 4):
            with pytest.raises(P.PbsimError, match="no prepared unit"):
                ctx.dump_table(which)
        assert _census(ctx, 5).tolist() == [0] * 12 and _census(ctx, 6).tolist() == [0] * 12
