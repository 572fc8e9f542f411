"""Random FIC-HMM models for the table builders and the four walkers: a generator, and a plain restatement of the
reference's cumulative-table build.  No GPU and no product code.

`errhmm_model(k)` / `qshmm_model(k)` give the text of model `k` in the shipped format (`<acc> IP|EP|TP <state> <values %.3e>`)
and the features it was built to contain, as {feature: [model classes that hold it]}.  Every value comes from
`random.Random(seed).random()` alone (no `choice`, `shuffle`, `randrange`: their streams have changed between Python
versions), a class's rows from a generator of its own, and the features sit in the model classes that most reads draw (the
top of the accuracy range of the case's --accuracy-mean).

`tables(text, method, skip_le)` restates the reference's build (pbsim.cpp:3715-3789 ERRHMM, resolution 1000; :2066-2142 QSHMM,
resolution 100; the start of it is tests/golden/make_models.py's cdf()): per accuracy class the initial-state table and its
modulus, per state both tables, both moduli and the deletion value, the highest state the tables name, and whether every
reachable modulus is the full resolution.  The running `end_wk` is ONE variable of the reference (pbsim.cpp:3615, :1974): an
expansion that skips every item reports what the one before it left, across rows and classes, and before the first class it
holds the modulus of the accuracy table.

`defined(t)` is the region in which the reference itself is well defined; a case that falls outside it is redrawn from
seed + 1000.  WHAT THE PRODUCT DOES OUTSIDE THIS REGION IS NOT PINNED BY THESE CASES.

`CASES` are the commands: a WGS leg each, a trans and a templ leg for some; tests/golden/make_model_fuzz.py runs the reference
on them and records digests (tests/golden/model_fuzz.json)."""
import functools
import hashlib
import math
import random

STATE_MAX = 50           # pbsim.cpp:43
QC_NUM = 94
COOP_MAX_STATES = 31     # kernels.h kCoopMaxStates: the ERRHMM wave walker's limit
QCOOP_MAX_STATES = 63    # kernels.h kQCoopMaxStates
ERR_SCALES = (0.995, 0.99, 0.97, 0.9)
QS_SCALES = (0.97, 0.93, 0.9)
FULL = 1.0003            # "sums to 1" after four significant digits per value: never below 0.9995


# ---- the restatement ------------------------------------------------------------------------------------------------------
def expand(vals, first, res, skip, end):
    """the reference's running-total expansion of vals (item numbers first, first + 1, ..): (table[0 .. res], 1-based, 0 where
    nothing was written; end_wk after it).  `end` is what the expansion before this one left."""
    table, start, total = [0] * (res + 1), 1, 0.0
    for i, v in enumerate(vals):
        if skip(v):
            continue
        total += v
        e = min(int(total * res + 0.5), res)
        for s in range(start, e + 1):
            table[s] = first + i
        end = e
        if e >= res:
            break
        start = e + 1
    return table, end


def accuracy_range(accuracy_mean):
    """(accuracy_min, accuracy_max, the modulus of the accuracy table, {class: share of the reads}), pbsim.cpp:3672-3706"""
    mean = accuracy_mean * 100
    hi = min(int(math.floor(mean * 1.05)), 100)
    lo = int(math.floor(mean * 0.75))
    tot = sum(math.exp(0.22 * a) for a in range(lo, hi + 1))
    table, end = expand([math.exp(0.22 * a) / tot for a in range(lo, hi + 1)], lo, 100000, lambda v: False, 0)
    share = {a: table[1:end + 1].count(a) / end for a in range(lo, hi + 1)}
    return lo, hi, end, share


def parse(text, method):
    """the model as set_errhmm (pbsim.cpp:5640) / set_qshmm (:5570) store it: {acc: {'ip': {state: v}, 'ep': {state: [v]},
    'tp': {state: {column: v}}, 'state_max': state of the last IP line}}"""
    m = {}
    for line in text.splitlines():
        t = line.split()
        c = m.setdefault(int(t[0]), {"ip": {}, "ep": {}, "tp": {}, "state_max": 0})
        j, vals = int(t[2]), [float(x) for x in t[3:]]
        assert 0 <= j <= STATE_MAX, "Q7 (states above STATE_MAX) is pinned elsewhere"
        if t[1] == "IP":
            c["ip"][j] = vals[0]
            c["state_max"] = j
        elif t[1] == "EP":
            c["ep"][j] = vals
        else:
            c["tp"][j] = {k + 1: v for k, v in enumerate(vals)}
    return m


def _closure(c, res):
    """the states a walk of the class can be in: those of the initial-state table's slots 1 .. init_rv, and of the transition
    tables' slots 1 .. tran_rv of every such state"""
    seen, todo = set(), [s for s in c["init"][1:c["init_rv"] + 1]]
    while todo:
        j = todo.pop()
        if j in seen or j == 0:
            seen.add(j)
            continue
        seen.add(j)
        st = c["states"].get(j)
        if st:
            todo += [s for s in set(st["tran"][1:st["tran_rv"] + 1]) if s not in seen]
    return seen


def _uni_ep(a):
    """uni_ep[a][0 .. 93], pbsim.cpp:558-578"""
    row = [0.0] * QC_NUM
    if a == 100:
        row[93] = 1.0
        return row
    qprob = [math.pow(10, q / -10) for q in range(QC_NUM)]
    prob = 1.0 - a / 100.0
    for q in range(QC_NUM):
        if prob == qprob[q]:
            row[q] = 1.0
            break
        if prob > qprob[q]:
            rate = (prob - qprob[q]) / (qprob[q - 1] - qprob[q])
            row[q - 1] = rate
            row[q] = 1 - rate
            break
    return row


def tables(text, method, skip_le=True, accuracy_mean=0.85):
    """The class tables the reference builds from the model text for the accuracy range of `accuracy_mean`.
    {'smax', 'lo', 'hi', 'res', 'classes': {acc: {'init_rv', 'init', 'states': {j: {'tran_rv', 'emis_rv', 'tran', 'emis',
    'del'}}, 'top', 'reach', 'full'}}, 'map': {drawn class: (mode, rate_mag, model class)} (ERRHMM), 'freq': {class without a
    model: (freq_rv, table)} (QSHMM), 'full': every reachable modulus of every class the range uses is `res`}.
    skip_le: the emission columns skipped are `<= 0` (WGS, pbsim.cpp:3743), else `== 0` (trans :4298, templ :4923)."""
    m = parse(text, method)
    lo, hi, end, _ = accuracy_range(accuracy_mean)
    zero = lambda v: v == 0
    err = method == "errhmm"
    res = 1000 if err else 100
    out = {"method": method, "lo": lo, "hi": hi, "res": res, "classes": {}, "map": {}, "freq": {},
           "acc_min": min(m), "acc_max": max(m), "model": m}
    if err:
        out["smax"] = max([1] + [c["state_max"] for c in m.values()] +
                          [k for c in m.values() for j in range(1, c["state_max"] + 1) for k, v in c["tp"].get(j, {}).items() if v != 0])
    else:
        out["smax"] = max([1] + [j for c in m.values() for j, v in c["ip"].items() if v != 0] +
                          [j for c in m.values() for j, r in c["ep"].items() if any(v != 0 for v in r)] +
                          [max(j, k) for c in m.values() for j, r in c["tp"].items() for k, v in r.items() if v != 0])
    for a in range(lo, hi + 1):
        if a not in m:
            if not err:
                table, end = expand(_uni_ep(a), 0, 1000, zero, end)
                out["freq"][a] = (end, table)
            continue
        src = m[a]
        n = src["state_max"] if err else STATE_MAX
        c = {"states": {}}
        c["init"], end = expand([src["ip"].get(j, 0.0) for j in range(1, n + 1)], 1, res, zero, end)
        c["init_rv"] = end
        for j in range(1, n + 1):
            ep = src["ep"].get(j, [])
            st = c["states"][j] = {}
            if err:
                ep = (ep + [0.0] * 4)[:4]
                st["del"] = int(ep[3] * 1000 + 0.5)
                st["emis"], end = expand(ep[:3], 0, res, (lambda v: v <= 0) if skip_le else zero, end)
            else:
                st["emis"], end = expand((ep + [0.0] * QC_NUM)[:QC_NUM], 0, res, zero, end)
            st["emis_rv"] = end
        for j in range(1, n + 1):
            row = src["tp"].get(j, {})
            st = c["states"][j]
            st["tran"], end = expand([row.get(k, 0.0) for k in range(1, STATE_MAX + 1)], 1, res, zero, end)
            st["tran_rv"] = end
        c["top"] = max([max(c["init"])] + [max(c["states"][j]["tran"]) for j in range(1, min(n, out["smax"]) + 1)])
        c["reach"] = _closure(c, res)
        c["full"] = c["init_rv"] == res and all(
            j in c["states"] and c["states"][j]["tran_rv"] == res and (err or c["states"][j]["emis_rv"] == res)
            for j in c["reach"] if j)
        out["classes"][a] = c
    if err:
        for a in range(lo, hi + 1):     # pbsim.cpp:3829-3833, :3837
            if a == 100:
                out["map"][a] = ("verbatim", 0, None)
            elif a in m:
                out["map"][a] = ("in", 0, a)
            elif a < out["acc_min"]:
                out["map"][a] = ("below", int((out["acc_min"] - a) / out["acc_min"] * 100), out["acc_min"])
            elif a > out["acc_max"]:
                out["map"][a] = ("above", int((a - out["acc_max"]) / (100 - out["acc_max"]) * 100), out["acc_max"])
            else:
                out["map"][a] = ("hole", 0, None)
        used = {mc for _, _, mc in out["map"].values() if mc is not None}
    else:
        used = set(out["classes"])
    out["used"] = used
    out["full"] = all(a in out["classes"] and out["classes"][a]["full"] for a in used)
    return out


def defined(t):
    """True where the reference's own walk of these tables is well defined"""
    err = t["method"] == "errhmm"
    if err and any(mode == "hole" for mode, _, _ in t["map"].values()):
        return False        # pbsim.cpp:3829-3833 assigns no rate_mag: the read before decides
    for a in t["used"]:
        c = t["classes"].get(a)
        if c is None:
            return False    # the model's acc_min / acc_max class lies outside the accuracy range: no table was built (:3709)
        if c["init_rv"] < 1 or 0 in c["init"][1:c["init_rv"] + 1]:
            return False    # rand() % 0 (pbsim.cpp:3854, :2216); state 0 has no rows
        for j in c["reach"]:
            st = c["states"].get(j)
            if st is None:
                return False    # ERRHMM: a state above state_max has no row, err_rand_value_tran is uninitialised (:3614, :3764)
            if st["tran_rv"] < 1 or 0 in st["tran"][1:st["tran_rv"] + 1]:
                return False    # rand() % 0 (pbsim.cpp:3857, :2219)
            if not err and st["emis_rv"] < 1:
                return False    # rand() % 0 (pbsim.cpp:2222)
    return True


def eligible(t, hp_del_bias=1.0):
    """whether a wave walker may take the model's tasks (engine.cpp coop_min_len)"""
    if t["method"] == "errhmm":
        return t["full"] and t["smax"] <= COOP_MAX_STATES
    return t["full"] and t["smax"] <= QCOOP_MAX_STATES and hp_del_bias == 1


# ---- the generator --------------------------------------------------------------------------------------------------------
def _ri(rng, a, b):
    return a + int(rng.random() * (b - a + 1))


def _pick(rng, seq):
    return seq[int(rng.random() * len(seq))]


def _fmt(vals):
    return " ".join("%.3e" % v for v in vals)


def _floor_row(rng, n, floor):
    """an initial-state row over n states, every state at least `floor`; sums to 1"""
    w = [x * x + 1e-3 for x in (rng.random() for _ in range(n))]
    s = sum(w)
    return [floor + (1.0 - floor * n) * x / s for x in w]


def _cycle_row(rng, n, j, stay, floor):
    """a sticky transition row over n states (j 0-based): stays with `stay`, steps to j + 1 (cyclically) and to up to four other
    states with at least `floor` each, exact zeros elsewhere; sums to 1"""
    if n == 1:
        return [1.0]
    row = [0.0] * n
    row[j] = stay
    picked = {(j + 1) % n}
    for _ in range(_ri(rng, 0, 4)):
        k = _ri(rng, 0, n - 1)
        if k != j:
            picked.add(k)
    w = {k: rng.random() + 1e-3 for k in sorted(picked)}
    room = 1.0 - stay - floor * len(w)
    tot = sum(w.values())
    for k, x in w.items():
        row[k] = floor + room * x / tot
    return row


# ERRHMM cases: seed, --accuracy-mean (None: the default 0.85), the model's classes, states of the two hot classes, the most
# states of any other class, whether IP / TP rows are scaled below 1, and the features built into the hot classes
ERR_SPECS = [
    dict(seed=101, mean=None, cls=(63, 89), n=(12, 1), cap=31, scaled=False,
         feats=("one_state", "clamp", "ip_leading_zeros", "emis_all_zero", "del_zero", "del_above_half")),
    dict(seed=102, mean=None, cls=(63, 89), n=(28, 30), cap=31, scaled=False,
         feats=("tp_only_state", "emis_mod0", "emis_mod1", "del_above_one")),
    dict(seed=103, mean=0.90, cls=(86, 94), n=(9, 14), cap=31, scaled=False, legs=True,
         feats=("emis_negative", "narrow_range", "del_zero")),
    dict(seed=104, mean=None, cls=(83, 87), n=(8, 5), cap=20, scaled=False, legs=True,
         feats=("emis_negative", "narrow_range", "emis_all_zero")),
    dict(seed=105, mean=None, cls=(63, 89), n=(7, 11), cap=12, scaled=True,
         feats=("scaled_rows", "emis_mod0", "ip_leading_zeros")),
    dict(seed=106, mean=None, cls=(63, 89), n=(47, 32), cap=50, scaled=False,
         feats=("clamp", "tp_only_state", "del_above_half")),
    dict(seed=107, mean=0.93, cls=(87, 99), n=(10, 6), cap=40, scaled=True, legs=True,
         feats=("scaled_rows", "emis_negative", "del_above_one")),
    dict(seed=108, mean=0.80, cls=(67, 93), n=(50, 1), cap=50, scaled=True,
         feats=("one_state", "scaled_rows", "emis_mod1", "del_above_half")),
    dict(seed=109, mean=0.97, cls=(93, 99), n=(9, 13), cap=24, scaled=True,
         feats=("narrow_range", "scaled_rows", "del_zero", "emis_all_zero")),
    dict(seed=110, mean=None, cls=(78, 92), n=(1, 20), cap=31, scaled=False,
         feats=("one_state", "ip_leading_zeros", "tp_only_state", "clamp", "del_above_one")),
    dict(seed=111, mean=None, cls=(63, 89), n=(45, 31), cap=50, scaled=False,
         feats=("emis_mod0", "emis_mod1", "emis_all_zero", "del_zero")),
    dict(seed=112, mean=0.88, cls=(86, 90), n=(16, 3), cap=20, scaled=True,
         feats=("narrow_range", "scaled_rows", "del_above_half", "ip_leading_zeros")),
    dict(seed=113, mean=None, cls=(80, 90), n=(22, 17), cap=31, scaled=False,
         feats=("clamp", "del_above_half", "emis_mod1")),
    # one state in every class: the smallest class blob there is (smax 1)
    dict(seed=114, mean=None, cls=(63, 89), n=(1, 1), cap=1, scaled=False, feats=("one_state",)),
]

# QSHMM cases: as above; nq: quality codes of the two hot classes; holes: classes inside the range without a model
QS_SPECS = [
    dict(seed=201, mean=None, cls=(63, 89), n=(10, 1), nq=(30, 12), cap=20, scaled=False,
         feats=("one_state", "code0", "clamp", "codes_few")),
    dict(seed=202, mean=None, cls=(63, 89), n=(50, 25), nq=(94, 41), cap=30, scaled=False,
         feats=("states_50", "codes_94", "codes_many", "ip_leading_zeros", "tp_only_state")),
    dict(seed=203, mean=None, cls=(63, 89), holes=(88,), n=(6, 9), nq=(1, 8), cap=16, scaled=False, legs=True,
         feats=("holes", "codes_1", "codes_few", "no_slot")),
    dict(seed=204, mean=0.82, cls=(80, 86), n=(16, 7), nq=(50, 33), cap=16, scaled=False,
         feats=("narrow_range", "code0", "ip_leading_zeros", "codes_many")),
    dict(seed=205, mean=None, cls=(63, 89), n=(12, 20), nq=(5, 27), cap=20, scaled=True, legs=True,
         feats=("scaled_rows", "no_slot", "codes_few")),
    dict(seed=206, mean=None, cls=(63, 89), n=(50, 40), nq=(94, 36), cap=50, scaled=False, bias="2.5",
         feats=("states_50", "tp_only_state", "clamp", "codes_94")),
    dict(seed=207, mean=None, cls=(63, 89), holes=(87, 88), n=(14, 1), nq=(28, 31), cap=24, scaled=True,
         feats=("holes", "scaled_rows", "one_state")),
    dict(seed=208, mean=0.90, cls=(84, 92), n=(11, 5), nq=(37, 1), cap=18, scaled=True,
         feats=("narrow_range", "scaled_rows", "codes_1", "code0")),
    dict(seed=209, mean=None, cls=(63, 89), n=(1, 19), nq=(26, 39), cap=30, scaled=False, bias="7",
         feats=("ip_leading_zeros", "clamp", "no_slot", "one_state")),
    dict(seed=210, mean=0.95, cls=(85, 99), holes=(97,), n=(31, 12), nq=(60, 45), cap=31, scaled=False,
         feats=("codes_many", "tp_only_state", "holes")),
    dict(seed=211, mean=None, cls=(75, 89), n=(33, 8), nq=(2, 24), cap=40, scaled=True,
         feats=("codes_few", "scaled_rows", "ip_leading_zeros", "narrow_range")),
    dict(seed=212, mean=None, cls=(63, 89), n=(13, 21), nq=(34, 94), cap=28, scaled=False, bias="10",
         feats=("codes_94", "code0", "clamp", "no_slot")),
    dict(seed=213, mean=None, cls=(63, 89), n=(50, 4), nq=(29, 1), cap=50, scaled=False,
         feats=("codes_1", "states_50")),
]


def hot_classes(spec):
    """the two model classes that most reads use: the top of the accuracy range (class 100 is copied verbatim, no walk), or the
    model's highest class where the range goes beyond it; never a hole"""
    _, hi, _, _ = accuracy_range(spec["mean"] or 0.85)
    top = min(hi, 99, spec["cls"][1])
    out = []
    while len(out) < 2:
        if top not in spec.get("holes", ()):
            out.append(top)
        top -= 1
    return out


def _err_text(spec, seed):
    feats, (h1, h2) = set(spec["feats"]), hot_classes(spec)
    where = {}
    lines = []
    for acc in range(spec["cls"][0], spec["cls"][1] + 1):
        rng = random.Random(seed * 1000 + acc)
        hot = acc in (h1, h2)
        n = spec["n"][(h1, h2).index(acc)] if hot else _ri(rng, 1, spec["cap"])
        big = hot and n >= 5            # features that need several states go to the hot class that has them
        scale = (lambda: _pick(rng, ERR_SCALES)) if spec["scaled"] and (hot or rng.random() < 0.7) else (lambda: FULL)
        mark = lambda f: where.setdefault(f, []).append(acc)
        if hot and spec["scaled"]:
            mark("scaled_rows")
        if n == 1 and hot:
            mark("one_state")
        ip = _floor_row(rng, n, 0.004)
        if big and "ip_leading_zeros" in feats:
            ip[0] = ip[1] = 0.0
            ip[3] = 0.0                 # and one exact zero inside the row
            mark("ip_leading_zeros")
        tp_only = n if big and "tp_only_state" in feats else 0
        if tp_only:
            ip[n - 1] = 0.0             # state n: no initial weight; the cycle's step n - 1 -> n reaches it
            mark("tp_only_state")
        f = 1.08 if big and "clamp" in feats else scale()
        if big and "clamp" in feats:
            mark("clamp")
        s = sum(ip)
        ip = [f * x / s for x in ip]
        for j in range(n):
            lines.append("%d IP %d %.3e" % (acc, j + 1, ip[j]))
        for j in range(n):
            e = (100 - acc) / 100.0
            sub, ins, dele = e * (0.02 + 0.28 * rng.random()), e * (0.2 + rng.random()), e * (0.1 + 0.8 * rng.random())
            if rng.random() < 0.15:
                sub = 0.0
            row = [max(0.05, 1.0 - sub - ins - dele), sub, ins, dele]
            if big:
                # states 1 .. 5 of the hot class: every one gets initial weight or a cycle step
                if "emis_all_zero" in feats and j == (0 if acc == h1 else 1):
                    row = [0.0, 0.0, 0.0, dele]                # inherits end_wk: of the initial table (state 1) or of state 1
                    mark("emis_all_zero")
                if "emis_mod0" in feats and j == 2:
                    row = [1e-4, 1e-4, 1e-4, dele]             # 0.3 / 1000 rounds to modulus 0: rand() % 3
                    mark("emis_mod0")
                if "emis_mod1" in feats and j == 3:
                    row = [2e-4, 5e-4, 0.0, dele] if acc == h1 else [6e-4, 1e-4, 1e-4, dele]   # modulus 1: slot 1 is sub | match
                    mark("emis_mod1")
                if "emis_negative" in feats and j == (1 if acc == h1 else 0):
                    row = [0.9, -2e-3, 0.05, dele] if acc == h1 else [0.85, 0.04, -1.5e-3, dele]
                    mark("emis_negative")
                if "del_zero" in feats and j == 4:
                    row[3] = 0.0
                    mark("del_zero")
                if "del_above_half" in feats and j == 0:
                    row[3] = 0.6
                    mark("del_above_half")
                if "del_above_one" in feats and j == 4:
                    row[3] = 1.2                               # every base this state meets is deleted
                    mark("del_above_one")
            lines.append("%d EP %d %s" % (acc, j + 1, _fmt(row)))
        for j in range(n):
            stay = 0.5 + 0.45 * rng.random()
            if big and "del_above_one" in feats and j == 4:
                stay = 0.2                                     # the all-deleting state is left soon
            row = _cycle_row(rng, n, j, stay, 0.004)
            f = 1.08 if big and "clamp" in feats and j % 3 == 0 else scale()
            row = [f * x for x in row]
            if tp_only and j == 0 and f >= 1.0:
                # a column past state_max behind a row that is already full: never reached by the expansion (it breaks at
                # 1000), seen by whoever sizes the tables from the TP columns
                row += [0.0] * (min(spec["cap"], n + 3) - n - 1) + [1e-3]
            lines.append("%d TP %d %s" % (acc, j + 1, _fmt(row)))
    if "narrow_range" in feats:
        where["narrow_range"] = [h1]
    return "\n".join(lines) + "\n", where


def _qs_text(spec, seed):
    feats, (h1, h2) = set(spec["feats"]), hot_classes(spec)
    where = {}
    lines = []
    for acc in range(spec["cls"][0], spec["cls"][1] + 1):
        if acc in spec.get("holes", ()):
            continue
        rng = random.Random(seed * 1000 + acc)
        hot = acc in (h1, h2)
        n = spec["n"][(h1, h2).index(acc)] if hot else _ri(rng, 1, spec["cap"])
        nq = spec["nq"][(h1, h2).index(acc)] if hot else _ri(rng, 20, 44)
        big = hot and n >= 5
        scale = (lambda: _pick(rng, QS_SCALES)) if spec["scaled"] and (hot or rng.random() < 0.7) else (lambda: 1.0)
        mark = lambda f: where.setdefault(f, []).append(acc)
        if hot:
            for f, yes in (("scaled_rows", spec["scaled"]), ("one_state", n == 1), ("states_50", n == 50), ("codes_1", nq == 1),
                           ("codes_94", nq == 94), ("codes_few", nq < 24), ("codes_many", nq > 40)):
                if yes and f in feats:
                    mark(f)
        ip = _floor_row(rng, n, 0.012)
        if big and "ip_leading_zeros" in feats:
            ip[0] = ip[1] = 0.0
            mark("ip_leading_zeros")
        if big and "tp_only_state" in feats:
            ip[n - 1] = None            # no IP line at all: the state is named by TP columns only
            mark("tp_only_state")
        if big and "no_slot" in feats:
            ip[2] = None
        f = 1.1 if big and "clamp" in feats else scale()
        s = sum(x for x in ip if x)
        for j in range(n):
            if ip[j] is not None:
                lines.append("%d IP %d %.3e" % (acc, j + 1, f * ip[j] / s))
            elif j == 2:
                lines.append("%d IP %d %.3e" % (acc, j + 1, 1e-3))     # 0.1 of a slot: the state has an IP entry and no slot
        for j in range(n):
            low = hot and "code0" in feats
            centre = rng.random() * 2 if low else 2 + rng.random() * max(nq - 5, 0)
            width = 1.0 + 3.0 * rng.random()
            w = [1.0 / (1.0 + ((q - centre) / width) * ((q - centre) / width) * ((q - centre) / width) * ((q - centre) / width))
                 for q in range(nq)]        # a bell from + - * / alone: the same digits under every libm
            if not low and nq > 1:
                w[0] = 0.0
            tiny = int(centre) if big and "no_slot" in feats and j < 3 and nq >= 5 else None
            if tiny is not None:
                w[tiny] = 0.0
            s = sum(w)
            f = 1.1 if big and "clamp" in feats and j % 2 == 0 else scale()
            row = [f * x / s for x in w]
            if tiny is not None:
                row[tiny] = 1e-4                                   # a code inside the row that rounds to no slot
                mark("no_slot")
            lines.append("%d EP %d %s" % (acc, j + 1, _fmt(row)))
        if low and hot:
            mark("code0")
        for j in range(n):
            row = _cycle_row(rng, n, j, 0.4 + 0.4 * rng.random(), 0.02)
            f = 1.1 if big and "clamp" in feats and j % 3 == 0 else scale()
            lines.append("%d TP %d %s" % (acc, j + 1, _fmt([f * x for x in row])))
        if big and "clamp" in feats:
            mark("clamp")
    if "narrow_range" in feats:
        where["narrow_range"] = [h1]
    if "holes" in feats:
        where["holes"] = list(spec["holes"])
    return "\n".join(lines) + "\n", where


def _model(method, k):
    spec = (ERR_SPECS if method == "errhmm" else QS_SPECS)[k]
    seed = spec["seed"]
    while True:
        text, where = (_err_text if method == "errhmm" else _qs_text)(spec, seed)
        if method == "errhmm":
            ok = all(defined(tables(text, method, le, spec["mean"] or 0.85)) for le in (True, False))
        else:
            ok = defined(tables(text, method, True, spec["mean"] or 0.85))
        if ok:
            return text, where
        seed += 1000


@functools.lru_cache(maxsize=None)
def errhmm_model(k):
    """(the text of ERRHMM model k, {feature: [model classes built to hold it]})"""
    return _model("errhmm", k)


@functools.lru_cache(maxsize=None)
def qshmm_model(k):
    """(the text of QSHMM model k, {feature: [model classes built to hold it]})"""
    return _model("qshmm", k)


def model_sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


# ---- the cases ------------------------------------------------------------------------------------------------------------
SHORT = ["--length-mean", "1200", "--length-sd", "900"]
BIASES = ("1", "2.5", "7", "10")      # 10 is the most the reference accepts ("Acceptable range is 1-10")
RATIOS = ("6:55:39", "39:24:36", "20:30:50", "5:10:85")
MODEL = "FUZZ-MODEL"                  # stands for the path the model text was written to (args_for)


def _case(method, k, spec):
    opt = "--" + method
    common = ["--method", method, opt, MODEL, "--pass-num", str(1 + (k + (method == "qshmm")) % 3)]
    if method == "errhmm":
        bias = BIASES[k % 4]
    else:
        bias = spec.get("bias", "1")
        common += ["--difference-ratio", RATIOS[k % 4]]
    if bias != "1":
        common += ["--hp-del-bias", bias]
    if spec["mean"]:
        common += ["--accuracy-mean", "%.2f" % spec["mean"]]
    seed = spec["seed"] * 10
    glen, depth = 200_000 + 25_000 * (k % 5), ("2", "2.5", "3")[k % 3]
    if spec.get("holes") or spec["cls"][1] - spec["cls"][0] < 26:
        glen, depth = 300_000, "3"      # the classes below the top of the range must get their reads too
    legs = {"wgs": ["--strategy", "wgs"] + common + ["--genome", "INPUT:synth_%d_%d.fa" % (glen, 70 + k), "--depth", depth,
                                                     "--seed", str(seed)] + SHORT}
    if spec.get("legs"):
        legs["trans"] = ["--strategy", "trans"] + common + ["--transcript", "INPUT:tiny.transcript", "--seed", str(seed + 1)]
        legs["templ"] = ["--strategy", "templ"] + common + ["--template", "INPUT:tiny.template", "--seed", str(seed + 2)]
    return dict(method=method, k=k, spec=spec, legs=legs, hp_del_bias=float(bias), accuracy_mean=spec["mean"] or 0.85,
                # the wave walkers are eligible: full rows, few enough states, and for QSHMM the default --hp-del-bias
                eligible=(not spec["scaled"] and (method == "qshmm" and bias == "1" or
                                                  method == "errhmm" and max(spec["cap"], *spec["n"]) <= COOP_MAX_STATES)))


CASES = {}
for _k, _s in enumerate(ERR_SPECS):
    CASES["errhmm_%02d" % _k] = _case("errhmm", _k, _s)
for _k, _s in enumerate(QS_SPECS):
    CASES["qshmm_%02d" % _k] = _case("qshmm", _k, _s)


def model_of(case):
    c = CASES[case]
    return (errhmm_model if c["method"] == "errhmm" else qshmm_model)(c["k"])


def args_for(case, leg, model_file):
    """the command line of a case's leg with the model's path in it (INPUT: names are left to harness.resolve)"""
    return [model_file if a == MODEL else a for a in CASES[case]["legs"][leg]]


def write_model(case, directory):
    """writes the case's model text into `directory`; its path"""
    import os
    p = os.path.join(directory, case + ".model")
    with open(p, "w") as f:
        f.write(model_of(case)[0])
    return p
