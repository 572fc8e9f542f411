"""CPU-side checks (no GPU) of the generated models of tests/model_fuzz.py: the generator has not drifted from the digests'
models, every designed feature is really in the tables and gets reads, the oracle gives the reference's digests
(tests/golden/model_fuzz.json), and the class blobs the product's host build packs from each model equal the plain
restatement of the reference's build, word for word."""
import functools
import json
import os
import re

import numpy as np
import pytest

import harness
import model_fuzz as M
import pbsim3_amd as P
import product

ERR = sorted(c for c in M.CASES if M.CASES[c]["method"] == "errhmm")
QS = sorted(c for c in M.CASES if M.CASES[c]["method"] == "qshmm")
ERR_FEATURES = ["one_state", "scaled_rows", "clamp", "zeros_inside", "ip_leading_zeros", "tp_only_state", "emis_all_zero",
                "emis_mod0", "emis_mod1", "emis_negative", "del_zero", "del_above_half", "del_above_one", "narrow_range",
                "states_le_31", "states_gt_31"]
QS_FEATURES = ["codes_1", "codes_94", "codes_few", "codes_many", "code0", "one_state", "states_50", "scaled_rows", "clamp",
               "ip_leading_zeros", "tp_only_state", "holes", "narrow_range", "no_slot"]
MODES = {"in": 0, "below": 1, "above": 2, "verbatim": 3}       # modes.h ErrMode


def load_json():
    with open(os.path.join(harness.GOLDEN, "model_fuzz.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fuzz_models"))


@functools.lru_cache(maxsize=None)
def restated(case, skip_le=True):
    c = M.CASES[case]
    return M.tables(M.model_of(case)[0], c["method"], skip_le, c["accuracy_mean"])


def params(case, model_file):
    return product.params_from_args(harness.resolve(M.args_for(case, "wgs", model_file)))


# ---- the model text -------------------------------------------------------------------------------------------------------
def test_there_are_enough_cases_of_each_kind():
    assert len(ERR) >= 12 and len(QS) >= 12
    for cases, least in ((ERR, 3), (QS, 2)):
        assert sum(M.CASES[c]["eligible"] for c in cases) >= 4
        assert sum(set(M.CASES[c]["legs"]) == {"wgs", "trans", "templ"} for c in cases) >= least
    for c in ERR:
        if "emis_negative" in M.CASES[c]["spec"]["feats"]:
            assert set(M.CASES[c]["legs"]) == {"wgs", "trans", "templ"}, c
    for c, v in M.CASES.items():
        a = v["legs"]["wgs"]
        glen = int(re.fullmatch(r"INPUT:synth_(\d+)_\d+\.fa", a[a.index("--genome") + 1]).group(1))
        assert 200_000 <= glen <= 300_000 and 2 <= float(a[a.index("--depth") + 1]) <= 3, c
        assert a[a.index("--pass-num") + 1] in ("1", "2", "3") and "--seed" in a, c
        assert (v["method"] == "qshmm") == ("--difference-ratio" in a), c
        if v["method"] == "qshmm" and v["eligible"]:
            assert "--hp-del-bias" not in a, c
    assert {M.CASES[c]["hp_del_bias"] for c in ERR} == {1.0, 2.5, 7.0, 10.0}
    assert sum(0.80 <= M.CASES[c]["accuracy_mean"] <= 0.97 and "--accuracy-mean" in M.CASES[c]["legs"]["wgs"] for c in M.CASES) >= 6


@pytest.mark.parametrize("case", ERR + QS)
def test_model_text_is_the_one_the_digests_were_made_from(case):
    gold = load_json()
    text, _ = M.model_of(case)
    for leg in M.CASES[case]["legs"]:
        assert M.model_sha(text) == gold[f"{case}/{leg}"]["model_sha256"], (case, leg)
    for line in text.splitlines():
        assert re.fullmatch(r"\d+ (IP|EP|TP) \d+( -?\d\.\d{3}e[-+]\d\d+)+", line), line
    t = [restated(case)] + ([restated(case, False)] if case in ERR else [])
    assert all(M.defined(x) for x in t), case


# ---- the census -----------------------------------------------------------------------------------------------------------
def _reachable(t, a):
    c = t["classes"][a]
    return [(j, c["states"][j], t["model"][a]) for j in sorted(c["reach"])]


def _ep(src, j, n):
    return (src["ep"].get(j, []) + [0.0] * n)[:n]


ERR_DETECT = {
    "one_state": lambda t, a: t["model"][a]["state_max"] == 1 and t["classes"][a]["reach"] == {1},
    "scaled_rows": lambda t, a: not t["classes"][a]["full"],
    "clamp": lambda t, a: sum(t["model"][a]["ip"].values()) > 1.0005 and any(
        sum(t["model"][a]["tp"][j].values()) > 1.0005 for j, _, _ in _reachable(t, a)),
    "ip_leading_zeros": lambda t, a: t["model"][a]["ip"][1] == 0 and t["model"][a]["ip"][2] == 0 and t["classes"][a]["init"][1] > 2,
    "tp_only_state": lambda t, a: any(src["ip"][j] == 0 for j, _, src in _reachable(t, a)) and
    max(k for r in t["model"][a]["tp"].values() for k, v in r.items() if v != 0) > t["model"][a]["state_max"],
    "emis_all_zero": lambda t, a: any(_ep(src, j, 3) == [0, 0, 0] and st["emis_rv"] > 1 for j, st, src in _reachable(t, a)),
    "emis_mod0": lambda t, a: any(st["emis_rv"] == 0 for _, st, _ in _reachable(t, a)),
    "emis_mod1": lambda t, a: any(st["emis_rv"] == 1 and any(_ep(src, j, 3)) for j, st, src in _reachable(t, a)),
    "emis_negative": lambda t, a: any(min(_ep(src, j, 3)) < 0 and _ep(src, j, 3)[0] > 0 for j, _, src in _reachable(t, a)),
    "del_zero": lambda t, a: any(st["del"] == 0 for _, st, _ in _reachable(t, a)),
    "del_above_half": lambda t, a: any(500 < st["del"] <= 1000 for _, st, _ in _reachable(t, a)),
    "del_above_one": lambda t, a: any(st["del"] > 1000 for _, st, _ in _reachable(t, a)),
    "narrow_range": lambda t, a: 5 <= t["acc_max"] - t["acc_min"] + 1 < 27 and
    len({mag for mode, mag, _ in t["map"].values() if mode in ("below", "above")}) >= 3,
}
QS_DETECT = {
    "codes_1": lambda t, a: all(len(r) == 1 for r in t["model"][a]["ep"].values()),
    "codes_94": lambda t, a: all(len(r) == 94 for r in t["model"][a]["ep"].values()),
    "codes_few": lambda t, a: all(len(r) < 24 for r in t["model"][a]["ep"].values()),
    "codes_many": lambda t, a: all(len(r) > 40 for r in t["model"][a]["ep"].values()),
    "code0": lambda t, a: any(src["ep"][j][0] > 0 and 0 in st["emis"][1:st["emis_rv"] + 1] for j, st, src in _reachable(t, a)),
    "one_state": lambda t, a: t["classes"][a]["reach"] == {1},
    "states_50": lambda t, a: 50 in t["classes"][a]["reach"],
    "scaled_rows": lambda t, a: not t["classes"][a]["full"],
    "clamp": lambda t, a: sum(t["model"][a]["ip"].values()) > 1.005 and any(
        sum(src["ep"][j]) > 1.005 and sum(src["tp"][j].values()) > 1.005 for j, _, src in _reachable(t, a)),
    "ip_leading_zeros": lambda t, a: t["model"][a]["ip"][1] == 0 and t["model"][a]["ip"][2] == 0 and t["classes"][a]["init"][1] > 2,
    "tp_only_state": lambda t, a: any(j not in src["ip"] for j, _, src in _reachable(t, a)),
    "holes": lambda t, a: a in t["freq"] and t["acc_min"] < a < t["acc_max"],
    "narrow_range": lambda t, a: (t["lo"] < t["acc_min"] or t["hi"] > t["acc_max"]) and t["freq"],
    "no_slot": lambda t, a: any(v != 0 and q not in st["emis"][1:] for j, st, src in _reachable(t, a)
                                for q, v in enumerate(src["ep"][j])) and
    any(v != 0 and j not in t["classes"][a]["init"] for j, v in t["model"][a]["ip"].items()),
}


def _features(case):
    """{feature: model classes} of a case: what the generator says it built, and what every case has by construction"""
    t, where = restated(case), dict(M.model_of(case)[1])
    if case in ERR:
        hot = M.hot_classes(M.CASES[case]["spec"])
        # exact zeros between a transition row's non-zero columns
        where["zeros_inside"] = [a for a in hot if any(
            0 in [r.get(k, 0.0) for k in range(min(k for k, v in r.items() if v), max(k for k, v in r.items() if v))]
            for r in t["model"][a]["tp"].values())]
        n = {a: t["model"][a]["state_max"] for a in t["used"]}
        where["states_le_31"] = [a for a in hot if n[a] <= M.COOP_MAX_STATES]
        where["states_gt_31"] = [a for a in hot if n[a] > M.COOP_MAX_STATES]
    return t, {f: v for f, v in where.items() if v}


def test_every_feature_occurs_in_two_cases():
    for cases, names in ((ERR, ERR_FEATURES), (QS, QS_FEATURES)):
        count = {f: 0 for f in names}
        for c in cases:
            t, where = _features(c)
            assert set(M.CASES[c]["spec"]["feats"]) <= set(where), (c, set(M.CASES[c]["spec"]["feats"]) - set(where))
            for f in where:
                count[f] += 1
        assert all(v >= 2 for v in count.values()), count
    # 1 to 50 states and 1 to 94 codes: both ends and the middle
    n = {restated(c)["model"][a]["state_max"] for c in ERR for a in restated(c)["used"]}
    assert {1, 50} <= n and len(n) >= 25
    nq = {len(r) for c in QS for a in restated(c)["classes"] for r in restated(c)["model"][a]["ep"].values()}
    assert {1, 94} <= nq and len(nq) >= 25


@pytest.mark.parametrize("case", ERR + QS)
def test_designed_features_are_in_the_tables_and_get_reads(case, model_dir):
    """every feature is found in the restated tables of the classes the generator names, and those classes expect 20 reads or
    more together: the case's reads (depth x genome / mean of the product's length table) times the classes' share of the
    product's accuracy table, counting the reads of the classes below and above an ERRHMM model's range with the model class
    that serves them"""
    t, where = _features(case)
    p, a = params(case, M.write_model(case, model_dir))
    with P.Context(p, -1) as ctx:
        p2l = np.frombuffer(ctx.dump_table(0), dtype=np.int32)[1:]
        p2a = np.frombuffer(ctx.dump_table(1), dtype=np.uint8)[1:]
    assert (int(p2a.min()), int(p2a.max())) == (t["lo"], t["hi"])
    glen = int(re.fullmatch(r".*synth_(\d+)_\d+\.fa", a["--genome"]).group(1))
    reads = float(a["--depth"]) * glen / p2l.mean()
    share = np.bincount(p2a, minlength=101) / len(p2a)
    detect = ERR_DETECT if case in ERR else QS_DETECT
    for f, classes in where.items():
        if case in ERR:
            got = sum(share[d] for d, (_, _, mc) in t["map"].items() if mc in classes)
        else:
            got = sum(share[c] for c in classes)
        assert reads * got >= 20, (case, f, classes, reads * got)
        if f in detect:
            for c in classes:
                assert detect[f](t, c), (case, f, c)
    if case in ERR and "emis_negative" in where:
        assert restated(case, True)["classes"] != restated(case, False)["classes"]


# ---- the oracle against the reference's digests ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,leg", [(c, leg) for c in ERR + QS for leg in M.CASES[c]["legs"]])
def test_oracle_matches_the_reference_digests(case, leg, tmp_path, model_dir):
    gold = load_json()[f"{case}/{leg}"]["outputs"]
    outs = harness.run_oracle(M.args_for(case, leg, M.write_model(case, model_dir)), "philox", str(tmp_path))
    assert sorted(outs) == sorted(gold), (case, leg)
    for k, v in outs.items():
        assert (len(v), harness.sha(v)) == (gold[k]["bytes"], gold[k]["sha256"]), (case, leg, k)


# ---- the product's class blobs against the restatement --------------------------------------------------------------------
def product_blob(case, model_file, strategy):
    p, a = params(case, model_file)
    p.strategy = strategy
    with P.Context(p, -1) as ctx:
        (ctx.load_errhmm if case in ERR else ctx.load_qshmm)(model_file)
        blob = ctx.dump_table(2)
    return blob


def check_err_blob(case, blob, t):
    ncls = t["hi"] - t["lo"] + 1
    smax = t["smax"]
    emis_off = 64 + 32 * (smax + 1)
    init_off = emis_off + 16 * (smax + 1)
    stride = (init_off + 1000 + 1000 * smax + 15) // 16 * 16
    assert len(blob) == ncls * stride, (case, len(blob), ncls, stride)
    for a in range(t["lo"], t["hi"] + 1):
        b = blob[(a - t["lo"]) * stride:(a - t["lo"] + 1) * stride]
        hdr = [int(x) for x in np.frombuffer(b[:64], dtype=np.uint32)]
        mode, mag, mc = t["map"][a]
        assert (hdr[0], hdr[2], hdr[3], hdr[4], hdr[5]) == (smax, MODES[mode], mag, a, mc or 0), (case, a, hdr)
        if mc is None:
            continue
        c = t["classes"][mc]
        assert (hdr[1], hdr[6]) == (c["init_rv"], c["top"]), (case, a, hdr, c["init_rv"], c["top"])
        rows = np.frombuffer(b[64:emis_off], dtype=np.uint16).reshape(smax + 1, 16)
        em = np.frombuffer(b[emis_off:init_off], dtype=np.uint32).reshape(smax + 1, 4)
        assert list(b[init_off:init_off + 1000]) == c["init"][1:], (case, a, "init")
        for j in range(1, smax + 1):
            st = c["states"].get(j)
            tran = b[init_off + 1000 * j:init_off + 1000 * (j + 1)]
            if st is None:      # the class has fewer states than the widest one: an empty row
                assert not rows[j][:4].any() and not any(tran), (case, a, j)
                continue
            rv = st["emis_rv"]
            e0 = sum(1 for s in range(1, rv + 1) if st["emis"][s] == 0)
            e1 = sum(1 for s in range(1, rv + 1) if st["emis"][s] <= 1)
            assert [int(x) for x in rows[j][:4]] == [st["tran_rv"], rv, e0, e1], (case, a, j, rows[j][:4], st["tran_rv"], rv, e0, e1)
            assert list(tran) == st["tran"][1:], (case, a, j, "tran")
            # the default bias: hp 1 .. 10 -> 1, hp 11 -> 0 (Q1)
            assert (int(rows[j][4 + 1]), int(rows[j][4 + 11])) == (st["del"], 0), (case, a, j, "del")
            assert int(em[j][3]) == st["del"], (case, a, j)
            magic, shift, neg_d = int(em[j][0]), int(em[j][1]) & 0xff, int(em[j][1]) >> 8
            d = (1 << 24) - neg_d
            t0, t1 = int(em[j][2]) & 0xffff, int(em[j][2]) >> 16
            top = (2 ** 31 - 1) // d * d
            for z in (0, 1, d - 1, d, 999, 1000, 2 ** 31 - 1, top, top - d):
                r = (z + (((z * magic >> 32) >> shift) & 0xffffff) * neg_d) & 0xffffff     # what the walk kernels compute
                want = z % 3 if rv == 0 else st["emis"][z % rv + 1]     # pbsim.cpp:3865-3869
                assert (r >= t0) + (r >= t1) == want, (case, a, j, z, rv, d, t0, t1)


def check_qs_blob(case, blob, t):
    ncls = t["hi"] - t["lo"] + 1
    smax = t["smax"]
    init_off = (64 + 4 * (smax + 1) + 15) // 16 * 16
    tran_off = init_off + 100
    emis_off = tran_off + 100 * smax
    freq_off = (emis_off + 100 * smax + 15) // 16 * 16
    stride = (freq_off + 1000 + 15) // 16 * 16
    assert len(blob) == ncls * stride, (case, len(blob), ncls, stride)
    for a in range(t["lo"], t["hi"] + 1):
        b = blob[(a - t["lo"]) * stride:(a - t["lo"] + 1) * stride]
        hdr = [int(x) for x in np.frombuffer(b[:64], dtype=np.uint32)]
        assert (hdr[0], hdr[4]) == (smax, a), (case, a, hdr)
        c = t["classes"].get(a)
        if c is None:
            rv, table = t["freq"][a]
            assert (hdr[2], hdr[3]) == (0, rv) and list(b[freq_off:freq_off + 1000]) == table[1:], (case, a, "freq")
            continue
        assert (hdr[1], hdr[2], hdr[3], hdr[6]) == (c["init_rv"], 1, 0, c["top"]), (case, a, hdr, c["init_rv"], c["top"])
        assert list(b[init_off:init_off + 100]) == c["init"][1:], (case, a, "init")
        rv = np.frombuffer(b[64:64 + 4 * (smax + 1)], dtype=np.uint16).reshape(smax + 1, 2)
        for j in range(1, smax + 1):
            st = c["states"][j]
            assert (int(rv[j][0]), int(rv[j][1])) == (st["tran_rv"], st["emis_rv"]), (case, a, j)
            assert list(b[tran_off + 100 * (j - 1):tran_off + 100 * j]) == st["tran"][1:], (case, a, j, "tran")
            assert list(b[emis_off + 100 * (j - 1):emis_off + 100 * j]) == st["emis"][1:], (case, a, j, "emis")


@pytest.mark.parametrize("case", ERR)
def test_errhmm_blob_equals_the_restatement(case, model_dir):
    f = M.write_model(case, model_dir)
    blobs = {}
    for skip_le, strategy in ((True, P.STRATEGY_WGS), (False, P.STRATEGY_TRANS), (False, P.STRATEGY_TEMPL)):
        t = restated(case, skip_le)
        blobs[strategy] = product_blob(case, f, strategy)
        check_err_blob(case, blobs[strategy], t)
        assert M.eligible(t) == M.CASES[case]["eligible"], case
    if "emis_negative" in M.CASES[case]["spec"]["feats"]:      # `<= 0` against `== 0` really builds other tables here
        assert blobs[P.STRATEGY_WGS] != blobs[P.STRATEGY_TRANS]
    assert blobs[P.STRATEGY_TRANS] == blobs[P.STRATEGY_TEMPL]


@pytest.mark.parametrize("case", QS)
def test_qshmm_blob_equals_the_restatement(case, model_dir):
    f = M.write_model(case, model_dir)
    t = restated(case)
    for strategy in (P.STRATEGY_WGS, P.STRATEGY_TRANS):
        check_qs_blob(case, product_blob(case, f, strategy), t)
    assert M.eligible(t, M.CASES[case]["hp_del_bias"]) == M.CASES[case]["eligible"], case


def test_errhmm_model_with_a_hole_is_refused_and_the_context_goes_on(model_dir, tmp_path):
    text, _ = M.model_of(ERR[0])
    holed = tmp_path / "holed.model"
    holed.write_text("".join(line + "\n" for line in text.splitlines() if not line.startswith("80 ")))
    assert not M.defined(M.tables(holed.read_text(), "errhmm"))
    good = M.write_model(ERR[0], model_dir)
    with P.Context(params(ERR[0], good)[0], -1) as ctx:
        ctx.load_errhmm(str(holed))
        with pytest.raises(P.PbsimError, match="no table for an accuracy class inside its own range"):
            ctx.dump_table(2)
        ctx.load_errhmm(good)
        check_err_blob(ERR[0], ctx.dump_table(2), restated(ERR[0]))
