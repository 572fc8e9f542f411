"""The rule of pbsim_bam_lift in plain Python: the records of an aligned BAM that lie on a variant genome, placed on the original
genome through the variant genome's origin maps.  It shares no code with the product and works on the inflated stream's bytes.

    lift_stream(stream, genome, origins, ref_name=None) -> (the lifted inflated stream, result)
    report(result)                                        -> the report text
    lift_record(pos, ops, origin)                         -> None (unplaced) or (pos, ops, columns)
    check_origin(origin, l_ref)                           -> None, or (variant position, what is wrong)

genome: a list of (name, bases); origins: per genome record one int32 per variant base, as pbsim_genome_mutate and pbsim_vcf_apply
write it: o >= 0 a kept or substituted base of original position o, -1 - p a base inserted behind p, -2^31 a base inserted in front
of position 0.  A failure of the call raises LiftError with the words the product uses.
"""
import struct

COUNTS = ["records", "unaligned", "unsupported", "unplaced", "lifted", "moved", "no_seq", "long_cigar_in", "long_cigar_out"]
TOTALS = ["cols_in", "cols_out", "m", "ins", "del", "soft", "sub", "gap_del", "bases_to_ins", "dels_vanished", "bytes_in", "bytes_out"]
FRONT = -2 ** 31            # a base inserted in front of position 0
MAX_OPS = 65535             # more ops than this leave as <l_seq>S<span>N with the CG:B,I tag
M, I, D, N, S, H, P, EQ, X = range(9)


class LiftError(Exception):
    pass


def check_origin(origin, l_ref):
    """the first variant position that breaks rule 2, with what it breaks; None for a good map"""
    last = -1                                   # the last kept value
    for v, o in enumerate(origin):
        o = int(o)
        if o >= 0:
            if o >= l_ref:
                return v, "a kept base names position %d, and the original record has %d bases" % (o, l_ref)
            if o <= last:
                return v, "the kept bases' positions do not rise strictly"
            last = o
        elif o != (FRONT if last < 0 else -1 - last):
            return v, "an inserted base does not name the last kept base in front of it"
    return None


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def base_class(c):
    """of a prepared genome byte: A C G T, and 4 for every other code"""
    return "ACGT".find(chr(c)) if chr(c) in "ACGT" else 4


def nibble_class(n):
    return {1: 0, 2: 1, 4: 2, 8: 3}.get(n, 4)


def lift_record(pos, ops, origin):
    """pos and the resolved CIGAR as [(length, op code)] of a record without N or P ops on a variant record with this origin map.
    None: no M column is left.  Else (pos, ops, columns): the lifted position, the lifted CIGAR, and per column of the lifted core
    (kind M I D, original position of an M, query index of an M or I), with the counts of what happened on the way in a dict."""
    cols = []                                   # the input columns: (kind, variant position, query index)
    clip = {(S, 0): 0, (S, 1): 0, (H, 0): 0, (H, 1): 0}
    v, q = pos, 0
    for n, op in ops:
        if op in (M, EQ, X):
            cols += [(M, v + k, q + k) for k in range(n)]
            v, q = v + n, q + n
        elif op == I:
            cols += [(I, None, q + k) for k in range(n)]
            q += n
        elif op == D:
            cols += [(D, v + k, None) for k in range(n)]
            v += n
        elif op in (S, H):
            clip[(op, 1 if cols else 0)] += n   # in front of every column: the left clip, else the right one
            q += n if op == S else 0
    prev_kept, last = [], -1                    # prev_kept[v]: the origin of the nearest kept base below v, -1 without
    for o in origin:
        prev_kept.append(last)
        if o >= 0:
            last = int(o)
    out, have_m = [], False                     # the output columns: (kind, original position, query index, is a gap column)
    what = dict(gap_del=0, bases_to_ins=0, dels_vanished=0, cols_in=len(cols))
    q_total = q
    for kind, v, q in cols:
        o = int(origin[v]) if kind != I else None
        if kind != I and o >= 0 and have_m:     # rule 8: the original bases the variant genome deleted
            out += [(D, None, None, True)] * (o - 1 - prev_kept[v])
        if kind == M and o >= 0:
            out.append((M, o, q, False))
            have_m = True
        elif kind == M:
            out.append((I, None, q, False))
            what["bases_to_ins"] += 1
        elif kind == I:
            out.append((I, None, q, False))
        elif o >= 0:
            out.append((D, None, None, False))
        else:
            what["dels_vanished"] += 1
    ms = [k for k, c in enumerate(out) if c[0] == M]
    if not ms:
        return None
    core = out[ms[0]:ms[-1] + 1]
    # rule 9: in front of the first M and behind the last I becomes S and D is dropped: all query bases out there are S
    left, right = core[0][2], q_total - 1 - core[-1][2]
    what["gap_del"] = sum(1 for c in core if c[3])
    runs = []
    for c in core:
        if runs and runs[-1][1] == c[0]:
            runs[-1][0] += 1
        else:
            runs.append([1, c[0]])
    new = [(clip[(H, 0)], H), (left, S)] + [tuple(r) for r in runs] + [(right, S), (clip[(H, 1)], H)]
    new = [(n, op) for n, op in new if n > 0]
    what["soft"] = left + right
    return core[0][1], new, core, what


def _aux_fields(rec, at):
    """the aux fields of a record from byte `at` on as (tag, the field's bytes)"""
    out = []
    while at < len(rec):
        tag, t = bytes(rec[at:at + 2]), chr(rec[at + 2])
        if t in "AcC":
            n = 1
        elif t in "sS":
            n = 2
        elif t in "iIf":
            n = 4
        elif t in "ZH":
            n = rec.index(0, at + 3) + 1 - (at + 3)
        elif t == "B":
            each = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[chr(rec[at + 3])]
            n = 5 + each * struct.unpack_from("<I", rec, at + 4)[0]
        else:
            raise LiftError("an aux field of unknown type")
        out.append((tag, bytes(rec[at:at + 3 + n])))
        at += 3 + n
    return out


def _int_tag(tag, v):
    """an integer tag of the smallest type that holds the value, as the truth writer chooses it"""
    for t, fmt, lo, hi in (("C", "<B", 0, 255), ("S", "<H", 0, 65535), ("I", "<I", 0, 2 ** 32 - 1)):
        if lo <= v <= hi:
            return tag + t.encode() + struct.pack(fmt, v)
    raise LiftError("NM does not fit")


def rewrite_text(text, names, lengths):
    """the header text: an SO: value of @HD becomes `unsorted`, the LN: of the @SQ line of each reference its original length"""
    lines = text.split(b"\n")
    for k, line in enumerate(lines):
        f = line.split(b"\t")
        if k == 0 and f[0] == b"@HD":
            f = [b"SO:unsorted" if x.startswith(b"SO:") else x for x in f]
        elif f[0] == b"@SQ":
            sn = [x[3:] for x in f[1:] if x.startswith(b"SN:")]
            if sn and sn[0] in names:
                f = [f[0]] + [b"LN:%d" % lengths[names.index(sn[0])] if x.startswith(b"LN:") else x for x in f[1:]]
        lines[k] = b"\t".join(f)
    return b"\n".join(lines)


def lift_stream(stream, genome, origins, ref_name=None):
    stream = bytes(stream)
    genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(seq).replace(b"\n", b"").upper()) for nm, seq in genome]
    if len(origins) != len(genome):
        raise LiftError("one origin map per genome record")
    if stream[:4] != b"BAM\x01":
        raise LiftError("not a BAM file")
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    names, var_len = [], []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, at)[0]
        names.append(stream[at + 4:at + 4 + l_name - 1])
        var_len.append(struct.unpack_from("<i", stream, at + 4 + l_name)[0])
        at += 8 + l_name
    if ref_name is not None and n_ref != 1:
        raise LiftError("a name given to a file that has not exactly one reference")
    gnames = [nm for nm, _ in genome]
    rec_of = []                                 # the genome record of reference k
    for k, nm in enumerate(names):
        want = (ref_name.encode() if isinstance(ref_name, str) else ref_name) if ref_name is not None else nm
        if want not in gnames:
            raise LiftError("the genome has no record named \"%s\"" % want.decode())
        g = gnames.index(want)
        if var_len[k] != len(origins[g]):
            raise LiftError("the reference \"%s\" has l_ref %d in the file's header, and the origin map of the genome's record of that name "
                            "has %d bases: this is not the genome these reads came from" % (want.decode(), var_len[k], len(origins[g])))
        rec_of.append(g)
    for g in sorted(set(rec_of)):
        bad = check_origin(origins[g], len(genome[g][1]))
        if bad:
            raise LiftError("the origin map of \"%s\" is not one: variant position %d: %s" % (gnames[g].decode(), bad[0], bad[1]))
    new_len = [len(genome[g][1]) for g in rec_of]
    new_text = rewrite_text(text, names, new_len)
    head = b"BAM\x01" + struct.pack("<i", len(new_text)) + new_text + struct.pack("<i", n_ref)
    for k, nm in enumerate(names):
        head += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", new_len[k])
    res = {k: 0 for k in COUNTS + TOTALS}
    out = [head]
    while at < len(stream):
        size = struct.unpack_from("<I", stream, at)[0]
        rec = stream[at:at + 4 + size]
        at += 4 + size
        res["records"] += 1
        ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
        if flag & 4 or ref_id < 0 or ref_id >= n_ref or pos < 0 or n_cigar == 0:
            res["unaligned"] += 1
            out.append(rec)
            continue
        cig_at = 36 + l_name
        seq_at = cig_at + 4 * n_cigar
        qual_at = seq_at + (l_seq + 1) // 2
        aux = _aux_fields(rec, qual_at + l_seq)
        ops = [(x >> 4, x & 15) for x in struct.unpack_from("<%dI" % n_cigar, rec, cig_at)]
        long_in = False
        if n_cigar == 2 and ops[0] == (l_seq, S) and ops[1][1] == N:
            cg = [f for tag, f in aux if tag == b"CG" and f[2:4] == b"BI"]
            if cg:
                ops = [(x >> 4, x & 15) for x in struct.unpack_from("<%dI" % ((len(cg[0]) - 8) // 4), cg[0], 8)]
                long_in = True
        if any(op > X for _, op in ops):
            raise LiftError("a CIGAR op code above 8")
        if any(op in (N, P) for _, op in ops):
            res["unsupported"] += 1
            continue
        g = rec_of[ref_id]
        origin, bases = origins[g], genome[g][1]
        span_in = sum(n for n, op in ops if op in (M, D, EQ, X))
        query = sum(n for n, op in ops if op in (M, I, S, EQ, X))
        if pos + span_in > len(origin) or (l_seq != 0 and query != l_seq):
            raise LiftError("a record does not fit: its CIGAR runs past its reference, or its query length is not l_seq")
        got = lift_record(pos, ops, origin)
        if got is None:
            res["unplaced"] += 1
            continue
        new_pos, new_ops, core, what = got
        n_m = sum(1 for c in core if c[0] == M)
        n_i = sum(1 for c in core if c[0] == I)
        n_d = sum(1 for c in core if c[0] == D)
        sub = 0
        if l_seq:
            for kind, o, q, _ in core:
                if kind == M:
                    nib = (rec[seq_at + q // 2] >> (0 if q & 1 else 4)) & 15
                    rc = base_class(bases[o])
                    bc = rc if nib == 0 else nibble_class(nib)
                    sub += rc != 4 and bc != 4 and rc != bc
        big = len(new_ops) > MAX_OPS
        cigar = b"".join(struct.pack("<I", n << 4 | op) for n, op in new_ops)
        field = struct.pack("<II", l_seq << 4 | S, (n_m + n_d) << 4 | N) if big else cigar
        tags = b""
        if l_seq:
            tags += _int_tag(b"NM", sub + n_i + n_d)
        if big:
            tags += b"CGBI" + struct.pack("<I", len(new_ops)) + cigar
        tags += b"".join(f for tag, f in aux if tag not in (b"NM", b"CG"))
        body = struct.pack("<iiBBHHH", ref_id, new_pos, l_name, mapq, reg2bin(new_pos, new_pos + n_m + n_d), 2 if big else len(new_ops), flag)
        body += rec[20:cig_at] + field + rec[seq_at:qual_at + l_seq] + tags
        new = struct.pack("<I", len(body)) + body
        out.append(new)
        res["lifted"] += 1
        res["moved"] += new_pos != pos or new_ops != ops
        res["no_seq"] += l_seq == 0
        res["long_cigar_in"] += long_in
        res["long_cigar_out"] += big
        for k in ("cols_in", "gap_del", "bases_to_ins", "dels_vanished", "soft"):
            res[k] += what[k]
        res["cols_out"] += len(core)
        res["m"] += n_m
        res["ins"] += n_i
        res["del"] += n_d
        res["sub"] += sub
        res["bytes_in"] += len(rec)
        res["bytes_out"] += len(new)
    return b"".join(out), res


def report(res):
    names = COUNTS + TOTALS
    return ("#\t" + "\t".join(names) + "\nL\t" + "\t".join(str(res[k]) for k in names) + "\n").encode()
