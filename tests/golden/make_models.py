#!/usr/bin/env python3
"""Synthetic FIC-HMM model files for the parity cases that no shipped model reaches (missing 4).

Every model under /root/reference/data has initial / transition rows that sum to 1 within rounding, so the reference's
cumulative tables end at exactly 1000 (ERRHMM, pbsim.cpp:3715-3789) resp. 100 (QSHMM, :2066-2142) and its draws are
`rand() % 1000` / `% 100` everywhere.  The table builders accept any row: `err_rand_value_{init,tran}` and
`qc_rand_value_{init,emis,tran}` are whatever the cumulative sum rounds to.  These files make the other moduli and the
state counts beyond the wave walkers' limits real:

  SYNTH-ERRHMM-MOD.model     classes 66..92, 3-12 states, IP / TP rows scaled to 1.0 / 0.995 / 0.99 / 0.97 / 0.9
  SYNTH-ERRHMM-S35.model     classes 66..92, rows sum to 1; class 84 has 35 states, class 85 has 50 (= STATE_MAX, pbsim.cpp:43)
  SYNTH-QSHMM-MOD.model      classes 66..92, 4-20 states, 24 quality codes, IP / EP / TP rows scaled likewise

and the state-count limits of the wave walkers (k_walk_errhmm_coop / k_walk_qshmm_coop walk every start state a group of
eight columns could begin in, in chains of eight up to the class's `reach`, header word 6 of host_tables.cpp).  Rows sum to 1,
every state of a class can be reached (a cycle j -> j + 1 with a few per-mille at least), and each class's highest state is
the one it is designed to reach:

  SYNTH-ERRHMM-S31.model     classes 66..92, smax 31: reach 1, 8, 15, 16, 23, 24, 29, 30, 31 in classes 81..89
                             (two chains up to 15, three up to 23, four above), 3-12 states elsewhere
  SYNTH-ERRHMM-S32.model     the same classes and class 80 with 32 states: past kCoopMaxStates, the lane walker only
  SYNTH-QSHMM-S50.model      classes 63..92, smax 50: reach 7, 8, 15, 16, 23, 24, 31, 32, 39, 40, 47, 48, 50 in classes
                             77..89 (n_chains = (reach + 8) >> 3: both edges of 1 .. 7), 4-12 states elsewhere

Before it writes one of these, the generator restates the reference's cumulative-table build on the values as written
(pbsim.cpp:3715-3789, 2066-2142) and asserts the designed moduli and reach of every class.

The files are written in the shipped models' own format (`<acc> IP|EP|TP <state> <values %.3e>`, set_errhmm :5640,
set_qshmm :5570) and committed gzip-compressed next to them; the goldens come from running the reference on them
(make_golden.py).  Run only to regenerate."""
import gzip
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "models")
SCALES = [1.0, 0.995, 0.99, 0.97, 0.9]


def sticky_row(rng, n, j, stay):
    """a transition row over n states that stays in state j with probability `stay` (the shipped models are sticky)"""
    w = [rng.random() ** 3 for _ in range(n)]
    w[j] = 0.0
    s = sum(w) or 1.0
    row = [(1.0 - stay) * x / s for x in w]
    row[j] = stay if n > 1 else 1.0
    # a few exact zeros like the real files have tiny entries: the table builders skip `== 0` columns
    for k in range(n):
        if k != j and rng.random() < 0.2:
            row[j] += row[k]
            row[k] = 0.0
    return row


def fmt(vals):
    return " ".join("%.3e" % v for v in vals)


def errhmm(path, seed, states_of, scaled):
    rng = random.Random(seed)
    lines = []
    for acc in range(66, 93):
        n = states_of(acc, rng)
        ip = [rng.random() ** 2 for _ in range(n)]
        s = sum(ip)
        f = rng.choice(SCALES) if scaled else 1.0
        ip = [f * x / s for x in ip]
        for j in range(n):
            lines.append("%d IP %d %.3e" % (acc, j + 1, ip[j]))
        for j in range(n):
            # match | substitution | insertion (the cumulative table, :3741-3762) and the deletion threshold (:3740)
            err = (100 - acc) / 100.0
            sub, ins, dele = (err * rng.uniform(0.02, 0.3), err * rng.uniform(0.2, 1.2), err * rng.uniform(0.1, 0.9))
            if rng.random() < 0.15:
                sub = 0.0
            match = max(0.05, 1.0 - sub - ins - dele)
            lines.append("%d EP %d %s" % (acc, j + 1, fmt([match, sub, ins, dele])))
        for j in range(n):
            f = rng.choice(SCALES) if scaled else 1.0
            row = [f * x for x in sticky_row(rng, n, j, rng.uniform(0.5, 0.95))]
            lines.append("%d TP %d %s" % (acc, j + 1, fmt(row)))
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(("\n".join(lines) + "\n").encode())


def qshmm(path, seed):
    rng = random.Random(seed)
    lines = []
    nq = 24
    for acc in range(66, 93):
        n = 4 + (acc * 5) % 17
        ip = [rng.random() ** 2 for _ in range(n)]
        s = sum(ip)
        f = rng.choice(SCALES)
        for j in range(n):
            lines.append("%d IP %d %.3e" % (acc, j + 1, f * ip[j] / s))
        for j in range(n):
            centre = rng.uniform(2, nq - 3)
            w = [pow(2.718281828, -((q - centre) / rng.uniform(1.0, 4.0)) ** 2) for q in range(nq)]
            w[0] = 0.0  # quality 0 ('!') carries error probability 1: keep the reads non-degenerate
            s = sum(w)
            f = rng.choice(SCALES)
            lines.append("%d EP %d %s" % (acc, j + 1, fmt([f * x / s for x in w])))
        for j in range(n):
            f = rng.choice(SCALES)
            row = [f * x for x in sticky_row(rng, n, j, rng.uniform(0.4, 0.9))]
            lines.append("%d TP %d %s" % (acc, j + 1, fmt(row)))
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(("\n".join(lines) + "\n").encode())


# ---- the wave walkers' state-count limits ---------------------------------------------------------------------------------
S31_DESIGN = {81: 1, 82: 8, 83: 15, 84: 16, 85: 23, 86: 24, 87: 29, 88: 30, 89: 31}
S32_DESIGN = {**S31_DESIGN, 80: 32}
S50_DESIGN = {77: 7, 78: 8, 79: 15, 80: 16, 81: 23, 82: 24, 83: 31, 84: 32, 85: 39, 86: 40, 87: 47, 88: 48, 89: 50}


def cycle_row(rng, n, j, stay, floor):
    """a sticky transition row over n states (j is 0-based) that also steps to j + 1 (cyclically) with at least `floor`, so
    that every state of the class is reachable, and to a few other states with at least `floor` each; sums to 1"""
    if n == 1:
        return [1.0]
    row = [0.0] * n
    row[j] = stay
    nxt = (j + 1) % n
    others = [k for k in range(n) if k not in (j, nxt)]
    picked = rng.sample(others, min(len(others), rng.randint(0, 4)))
    w = {k: rng.random() for k in [nxt] + picked}
    room = 1.0 - stay - floor * len(w)
    assert room >= 0
    tot = sum(w.values())
    for k, x in w.items():
        row[k] = floor + room * x / tot
    return row


def floor_row(rng, n, floor):
    """an initial-state row over n states, every state at least `floor`; sums to 1"""
    w = [rng.random() ** 2 for _ in range(n)]
    s = sum(w)
    return [floor + (1.0 - floor * n) * x / s for x in w]


def cdf(vals, res, skip):
    """the reference's cumulative table over vals[0..]: (table[1..end] as 1-based indices into vals, end)"""
    table, start, total, end = [], 1, 0.0, 0
    for i, v in enumerate(vals):
        if skip(v):
            continue
        total += v
        end = min(int(total * res + 0.5), res)
        table += [i + 1] * (end - start + 1)
        if end >= res:
            break
        start = end + 1
    return table, end


def parse(path):
    """{acc: {'IP': {state: [values]}, 'EP': .., 'TP': ..}} of a written model file (the values as the reference reads them)"""
    out = {}
    with gzip.open(path, "rt") as f:
        for line in f:
            t = line.split()
            out.setdefault(int(t[0]), {"IP": {}, "EP": {}, "TP": {}})[t[1]][int(t[2])] = [float(x) for x in t[3:]]
    return out


def check_limits(path, res, design, filler):
    """restates the class tables the reference builds from the file (pbsim.cpp:3715-3789 ERRHMM, res 1000; :2066-2142 QSHMM,
    res 100) and asserts that every reachable modulus is `res` and every class reaches exactly its designed state"""
    m = parse(path)
    for acc, c in sorted(m.items()):
        n = len(c["IP"])
        ip = [c["IP"][j][0] for j in range(1, n + 1)]
        init, end = cdf(ip, res, lambda v: v == 0)
        assert end == res, (path, acc, "IP", end)
        seen = set(init)
        for j in range(1, n + 1):
            tab, end = cdf(c["TP"][j], res, lambda v: v == 0)
            assert end == res, (path, acc, "TP", j, end)
            seen |= set(tab)
            if res == 100:
                tab, end = cdf(c["EP"][j], res, lambda v: v == 0)
                assert end == res, (path, acc, "EP", j, end)
        want = design.get(acc, filler(acc))
        assert seen == set(range(1, want + 1)), (path, acc, sorted(set(range(1, want + 1)) - seen), max(seen), want)
    return m


def errhmm_limits(path, seed, design):
    lines = []
    filler = lambda acc: 3 + (acc * 7) % 10
    for acc in range(66, 93):
        rng = random.Random(seed * 1000 + acc)        # a class's rows do not depend on the other classes
        n = design.get(acc, filler(acc))
        ip = floor_row(rng, n, 0.004)
        for j in range(n):
            lines.append("%d IP %d %.3e" % (acc, j + 1, ip[j]))
        for j in range(n):
            err = (100 - acc) / 100.0
            sub, ins, dele = (err * rng.uniform(0.02, 0.3), err * rng.uniform(0.2, 1.2), err * rng.uniform(0.1, 0.9))
            lines.append("%d EP %d %s" % (acc, j + 1, fmt([max(0.05, 1.0 - sub - ins - dele), sub, ins, dele])))
        for j in range(n):
            lines.append("%d TP %d %s" % (acc, j + 1, fmt(cycle_row(rng, n, j, rng.uniform(0.5, 0.9), 0.004))))
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(("\n".join(lines) + "\n").encode())
    check_limits(path, 1000, design, filler)


def qshmm_limits(path, seed, design):
    lines = []
    nq = 24
    filler = lambda acc: 4 + (acc * 5) % 9
    for acc in range(63, 93):
        rng = random.Random(seed * 1000 + acc)
        n = design.get(acc, filler(acc))
        # a QSHMM table has 100 slots: a state needs a few per cent to hold one whatever the rounding of its neighbours
        ip = floor_row(rng, n, 0.015)
        for j in range(n):
            lines.append("%d IP %d %.3e" % (acc, j + 1, ip[j]))
        for j in range(n):
            centre = rng.uniform(2, nq - 3)
            w = [pow(2.718281828, -((q - centre) / rng.uniform(1.0, 4.0)) ** 2) for q in range(nq)]
            w[0] = 0.0
            s = sum(w)
            lines.append("%d EP %d %s" % (acc, j + 1, fmt([x / s for x in w])))
        for j in range(n):
            lines.append("%d TP %d %s" % (acc, j + 1, fmt(cycle_row(rng, n, j, rng.uniform(0.4, 0.8), 0.02))))
    with gzip.GzipFile(path, "wb", mtime=0) as g:
        g.write(("\n".join(lines) + "\n").encode())
    check_limits(path, 100, design, filler)


def main():
    errhmm(os.path.join(OUT, "SYNTH-ERRHMM-MOD.model.gz"), 41, lambda acc, rng: 3 + (acc * 7) % 10, True)
    errhmm(os.path.join(OUT, "SYNTH-ERRHMM-S35.model.gz"), 42,
           lambda acc, rng: 35 if acc == 84 else 50 if acc == 85 else 3 + (acc * 7) % 10, False)
    qshmm(os.path.join(OUT, "SYNTH-QSHMM-MOD.model.gz"), 43)
    errhmm_limits(os.path.join(OUT, "SYNTH-ERRHMM-S31.model.gz"), 44, S31_DESIGN)
    errhmm_limits(os.path.join(OUT, "SYNTH-ERRHMM-S32.model.gz"), 44, S32_DESIGN)
    qshmm_limits(os.path.join(OUT, "SYNTH-QSHMM-S50.model.gz"), 45, S50_DESIGN)


if __name__ == "__main__":
    main()
