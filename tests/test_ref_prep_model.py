"""The plain model of the reference preparation (ref_prep_model.py) against a per-base loop: the GPU test of the
preparation kernels (test_gpu_reference_prep.py) leans on the vectorised model, this guards the model.

hp_census_weighted (host_tables.cpp; the trans / templ deletion bias comes from it whenever --hp-del-bias is not 1) is
reached through tests/asan/hp_census_driver.cpp, built with host_tables.cpp like the table builders' driver, and must
count what the model counts."""
import subprocess

import numpy as np
import pytest

import ref_prep_model as M

ALPHABET = np.frombuffer(b"ACGTNacgtn" + bytes([0x80, 0xC4, 0xE9, 0xFF]), dtype=np.uint8)


def naive(raw, units, keep_first, flag):
    """one base at a time, no numpy: upper-case, walk every run to its end, class, census"""
    n = len(raw)
    up = []
    for i, b in enumerate(raw):
        unit_start = i == 0 or raw[i - 1] == 10
        if 97 <= b <= 122 and not (keep_first and unit_start):
            b -= 32
        up.append(b)
    hp = [0] * n
    i = 0
    while i < n:
        j = i
        while j + 1 < n and up[j + 1] == up[i]:
            j += 1
        r = j - i + 1
        nnum = 0
        for _ in range(r):          # the reference's counter: past 11 it is set back to 10
            nnum += 1
            if nnum > 11:
                nnum = 10
        v = 1 if up[i] == ord("N") else nnum
        for k in range(i, j + 1):
            hp[k] = v
        i = j + 1
    census = [0] * 12
    for b, v in zip(up, hp):
        if not (units and b == 10):
            census[v] += 1
    seq = [b | 0x80 if flag and v == 11 else b for b, v in zip(up, hp)]
    return seq, hp, census


def _random_record(rng, n):
    """random bytes of the alphabet with runs mixed in (half of the pieces are runs of 1..30)"""
    out = []
    while len(out) < n:
        b = int(ALPHABET[rng.integers(0, ALPHABET.size)])
        out += [b] * (int(rng.integers(1, 31)) if rng.random() < 0.5 else 1)
    return bytes(out[:n])


@pytest.mark.parametrize("units", [False, True])
def test_model_matches_per_base_loop(units):
    rng = np.random.default_rng(20 + units)
    for case in range(300):
        if units:
            us = [_random_record(rng, int(rng.integers(1, 60))) for _ in range(int(rng.integers(1, 5)))]
            raw, keep_first = M.concat_units(us), bool(case & 1)
        else:
            raw, keep_first = _random_record(rng, int(rng.integers(1, 201))), False
        flag = bool(case & 2)
        seq, hp, census = M.prepare(raw, units=units, keep_first=keep_first, flag=flag)
        want = naive(raw, units, keep_first, flag)
        assert (seq.tolist(), hp.tolist(), census.tolist()) == want, (case, raw)
        assert census.sum() == len(raw) - (raw.count(b"\n") if units else 0)


def test_known_answers():
    seq, hp, census = M.prepare(b"aAaAaAaAaAaAc" + b"N" * 5 + b"n" + b"G" * 11 + b"T" * 13, flag=True)
    assert bytes(seq) == b"A" * 12 + b"C" + b"N" * 6 + bytes([ord("G") | 0x80]) * 11 + bytes([ord("T") | 0x80]) * 13
    assert hp.tolist() == [10] * 12 + [1] + [1] * 6 + [11] * 24
    assert census.tolist() == [0, 7, 0, 0, 0, 0, 0, 0, 0, 0, 12, 24]
    # units: the kept first byte splits the run, the separator ends it and is not counted
    raw = M.concat_units([b"aAAAA", b"AAc", b"n"])
    seq, hp, census = M.prepare(raw, units=True, keep_first=True)
    assert bytes(seq) == b"aAAAA\nAAC\nn\n"
    assert hp.tolist() == [1, 4, 4, 4, 4, 1, 2, 2, 1, 1, 1, 1]
    assert census.tolist() == [0, 3, 2, 0, 4, 0, 0, 0, 0, 0, 0, 0]
    assert M.flag_mode(b"ACGT", 1) and not M.flag_mode(b"AC\x80", 1) and not M.flag_mode(b"ACGT", 3)



@pytest.mark.parametrize("keep_first", [0, 1])
def test_census_equals_hp_census_weighted(keep_first, tmp_path):
    """hp_census_weighted(unit, weight 1, keep_first) of host_tables.cpp, unit by unit: random strings of ACGTNacgtn and
    bytes >= 0x80 with runs mixed in, lengths 1..200, and the runs the rules turn on (11, 12, 13, N, a kept first byte)"""
    import test_host_sanitizers as S
    exe = S.build(tmp_path, "hp_census_driver", "host_tables.cpp")
    rng = np.random.default_rng(40 + keep_first)
    units = [_random_record(rng, int(rng.integers(1, 201))) for _ in range(300)]
    units += [b"a" + b"A" * 12, b"A" * 11, b"A" * 12, b"a" * 13, b"n" + b"N" * 20, b"N", b"n", b"\xc4" * 13, b"\xff" * 12 + b"\xe9",
              b"aAaAaAaAaAaA", b"G" * 4101, b"g" * 4102]
    path = tmp_path / "units.txt"
    path.write_bytes(M.concat_units(units))
    p = subprocess.run([exe, str(keep_first), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    rows = [[int(x) for x in line.split()] for line in p.stdout.splitlines()]
    assert len(rows) == len(units)
    for u, row in zip(units, rows):
        want = M.prepare(M.concat_units([u]), units=True, keep_first=bool(keep_first))[2].tolist()
        assert row == want, (keep_first, u)
