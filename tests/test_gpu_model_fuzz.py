"""The generated models of tests/model_fuzz.py through the walkers (GPU), byte for byte against the digests the reference
gave for them (tests/golden/model_fuzz.json): WGS through the ABI and through the job pipeline -- where a wave walker must
have run exactly when the restated tables say it may --, the trans and templ legs, and one context through a wide, a
50-state and a one-state model in turn.  Reads nothing but the JSON and the oracle built from oracle/pbsim_oracle.c."""
import pytest

import harness
import model_fuzz as M
import pbsim3_amd as P
import product
from test_gpu_parity import _cmp
from test_model_fuzz_cpu import ERR, QS, load_json, restated

pytestmark = pytest.mark.gpu

GOLD = load_json()


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("fuzz_models"))


def check(case, leg, outs, model_file, tmp_path):
    gold = GOLD[f"{case}/{leg}"]["outputs"]
    assert sorted(outs) == sorted(k for k in gold if not k.endswith((".ref", ".stderr"))), (case, leg, sorted(outs))
    if any((len(v), harness.sha(v)) != (gold[k]["bytes"], gold[k]["sha256"]) for k, v in outs.items()):
        want = harness.run_oracle(M.args_for(case, leg, model_file), "philox", str(tmp_path))
        _cmp(outs, want, f"{case}/{leg}")
        raise AssertionError(f"{case}/{leg}: the product equals the oracle and both differ from the reference's digests")


@pytest.mark.parametrize("case", ERR + QS)
def test_wgs_matches_the_reference_digests(case, model_dir, tmp_path):
    f = M.write_model(case, model_dir)
    outs, _ = product.run_wgs(harness.resolve(M.args_for(case, "wgs", f)))
    check(case, "wgs", outs, f, tmp_path)


@pytest.mark.parametrize("case", ERR + QS)
def test_job_pipeline_matches_the_reference_digests(case, model_dir, tmp_path):
    """a 4 MB scratch pool: many rounds.  An eligible case that never reached a wave walker would pass untested."""
    f = M.write_model(case, model_dir)
    outs, _, waves = product.run_wgs_job(harness.resolve(M.args_for(case, "wgs", f)), scratch_mb=4)
    check(case, "wgs", outs, f, tmp_path)
    assert (waves > 0) == M.eligible(restated(case), M.CASES[case]["hp_del_bias"]), (case, waves)


@pytest.mark.parametrize("case,leg", [(c, leg) for c in ERR + QS for leg in M.CASES[c]["legs"] if leg != "wgs"])
def test_trans_and_templ_legs_match_the_reference_digests(case, leg, model_dir, tmp_path):
    f = M.write_model(case, model_dir)
    p, a = product.params_from_args(harness.resolve(M.args_for(case, leg, f)))
    with P.Context(p, 0) as ctx:
        (ctx.load_errhmm if case in ERR else ctx.load_qshmm)(f)
        if leg == "trans":
            ctx.load_transcript_file(a["--transcript"])
        else:
            ctx.load_template_file(a["--template"])
        rt, mt = ctx.simulate_trans()
        if p.pass_num > 1:
            rt = ctx.sam_header() + rt
    check(case, leg, {".fq" if p.pass_num == 1 else ".sam": rt, ".maf": mt}, f, tmp_path)


def test_one_context_through_a_wide_a_50_state_and_a_one_state_model(model_dir):
    """a class blob of a smaller smax and stride leaves nothing of the one before it in the device tables: the same record
    after each load gives the bytes of a context that only ever saw that model"""
    cases = ["errhmm_00", "errhmm_05", "errhmm_13", "errhmm_00"]
    assert [restated(c)["smax"] for c in cases[:3]] == [28, 50, 1]
    files = [M.write_model(c, model_dir) for c in cases]
    p, a = product.params_from_args(harness.resolve(M.args_for(cases[0], "wgs", files[0])))
    assert p.hp_del_bias == 1
    rec = product.read_fasta(a["--genome"])[0]

    def one(ctx, f):
        ctx.load_errhmm(f)
        ctx.set_reference(rec, 1)
        return ctx.simulate_wgs()

    with P.Context(p, 0) as ctx:
        got = [one(ctx, f) for f in files]
    for c, f, g in zip(cases, files, got):
        with P.Context(p, 0) as ctx:
            want = one(ctx, f)
        assert g[0] == want[0] and g[1] == want[1], c
    assert len({g[0] for g in got}) == 3
