"""What the reference preparation (k_hp_breaks / k_hp_carry / k_hp_final) must make of a record, as plain numpy.

The rules (get_genome_seq, pbsim.cpp:1035-1065; the per-transcript pass, :4385-4409):

  * a-z become A-Z, every other byte stays.  With `keep_first` the first byte of every unit keeps its case.
  * a run is a maximal stretch of equal prepared bytes.  Units are concatenated with one line feed behind each; the
    line feed is a byte no unit holds, so it ends the run on either side of it.
  * the class of a run of r bases is r up to 11, beyond that 11 for odd r and 10 for even r (the counter is set back
    to 10 whenever it passes 11); a base whose prepared byte is N has class 1 whatever its run.
  * census[v] = bases of class v, v = 0..11; with `units` the line feeds are not counted.
  * the prepared sequence byte is the upper-cased byte, with 0x80 added where the class is 11 when `flag` holds.

Everything is vectorised (break positions, np.diff, np.repeat, np.bincount): a record of 4 Mbp costs milliseconds."""
import numpy as np

LF = 10
SLOTS = 12


def concat_units(units):
    """the units in load order, each followed by one line feed"""
    return b"".join(bytes(u) + b"\n" for u in units)


def flag_mode(raw, hp_del_bias):
    """bit 7 of the sequence bytes carries class == 11: the default bias, and no byte that uses bit 7 itself"""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    return hp_del_bias == 1 and not bool((a >= 0x80).any())


def prepare(raw, units=False, keep_first=False, flag=False):
    """-> (sequence bytes uint8[n], class uint8[n], census int64[12]) of the record `raw` (units: of concat_units())"""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    n = a.size
    assert n >= 1
    lower = (a >= ord("a")) & (a <= ord("z"))
    if keep_first:
        first = np.empty(n, dtype=bool)
        first[0] = True
        first[1:] = a[:-1] == LF
        lower &= ~first
    up = a.copy()
    up[lower] -= 32
    brk = np.flatnonzero(np.concatenate(([True], up[1:] != up[:-1])))
    runs = np.diff(np.concatenate((brk, [n])))
    cls = np.where(runs <= 11, runs, np.where(runs & 1, 11, 10))
    hp = np.repeat(cls, runs).astype(np.uint8)
    hp[up == ord("N")] = 1
    counted = hp[up != LF] if units else hp
    census = np.bincount(counted, minlength=SLOTS).astype(np.int64)
    seq = up.copy()
    if flag:
        seq[hp == 11] |= 0x80
    return seq, hp, census
