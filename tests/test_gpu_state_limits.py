"""The wave walkers at their state-count limits (tests/golden/make_models.py): k_walk_errhmm_coop walks two, three or four
chains of eight start states per lane (reach 15 | 16, 23 | 24, states 30 and 31), k_walk_qshmm_coop one to seven (reach
7 | 8 .. 47 | 48, 50), and a model of 32 states goes to the lane walker whole.  The reference's goldens of these models with
every task, no task and the default share on the wave walker -- checking which walker really ran -- and larger runs of the
wave walker against the lane walker, bytes and statistics."""
import pytest

import harness
import pbsim3_amd as P
import product
from cases import CASES, STATE_LIMIT
from test_gpu_coop import genome
from test_gpu_parity import MANIFEST

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("coop", ["0", "-1", None])
@pytest.mark.parametrize("case", sorted(STATE_LIMIT))
def test_state_limit_goldens_on_either_walker(case, coop, monkeypatch):
    """PBSIM_COOP_LEN 0: every task of a qualifying model on the wave walker; -1: none; unset: the default split, which gives
    a small batch (every batch of these cases) to the wave walker whole"""
    if coop is None:
        monkeypatch.delenv("PBSIM_COOP_LEN", raising=False)
    else:
        monkeypatch.setenv("PBSIM_COOP_LEN", coop)
    args = harness.resolve(CASES[case]["args"])
    outs, _, waves = product.run_wgs_job(args, scratch_mb=product.scratch_mb_for(case))
    gold = MANIFEST[f"{case}/philox"]
    assert sorted(outs) == sorted(k for k in gold if not k.endswith((".ref", ".stderr"))), (case, sorted(outs))
    for k, v in outs.items():
        assert len(v) == gold[k]["bytes"] and harness.sha(v) == gold[k]["sha256"], (case, coop, k)
    if coop == "-1" or STATE_LIMIT[case] in product.NO_WAVE_MODELS:
        assert waves == 0, (case, coop, waves)
    else:
        assert waves > 0, (case, coop, "the wave walker took no task")


def run(coop, monkeypatch, records, method, model, **kw):
    """one job through the product on `records`; (texts, statistics, wave-walker launches)"""
    if coop is None:
        monkeypatch.delenv("PBSIM_COOP_LEN", raising=False)
    else:
        monkeypatch.setenv("PBSIM_COOP_LEN", str(coop))
    p = P.default_params(strategy=P.STRATEGY_WGS, method=method, **kw)
    with P.Context(p, 0) as ctx:
        ctx.set_scratch_bytes(256 << 20)
        (ctx.load_errhmm if method == P.METHOD_ERR else ctx.load_qshmm)(harness.model_path(model))
        for r in records:
            ctx.job_add_record(r)
        outs, done = ctx.job_run()
        waves = ctx.prof_wave_launches()
    texts = {k: (bytes(v[0]), bytes(v[1])) for k, v in outs.items()}
    stats = {k: tuple(getattr(v[0], f[0]) for f in v[0]._fields_) + tuple(v[1:]) for k, v in done.items()}
    return texts, stats, waves


ERR, QS = P.METHOD_ERR, P.METHOD_QS
RUNS = {
    "s31_default": dict(method=ERR, model="SYNTH-ERRHMM-S31.model", seed=7, depth=8.0),
    "s31_pass3_hp_bias": dict(method=ERR, model="SYNTH-ERRHMM-S31.model", seed=5, depth=5.0, pass_num=3, hp_del_bias=2.0,
                              len_mean=3000.0, len_sd=2500.0),
    "s31_high_accuracy": dict(method=ERR, model="SYNTH-ERRHMM-S31.model", seed=11, depth=8.0, accuracy_mean=0.90),
    "s50_default": dict(method=QS, model="SYNTH-QSHMM-S50.model", seed=7, depth=8.0),
    "s50_pass3": dict(method=QS, model="SYNTH-QSHMM-S50.model", seed=9, depth=4.0, pass_num=3, len_mean=4000.0, len_sd=3000.0),
    "s50_deletion_heavy": dict(method=QS, model="SYNTH-QSHMM-S50.model", seed=3, depth=8.0, sub_ratio=5, ins_ratio=10,
                               del_ratio=85),
}


def records():
    return [genome(600_000, 1), genome(300_000, 2)]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_state_limit_wave_walker_matches_lane_walker(name, monkeypatch):
    """every byte and every statistic, whatever share of the tasks the wave walker takes"""
    recs = records()
    want = run(-1, monkeypatch, recs, **RUNS[name])
    assert want[2] == 0
    assert sum(len(a) + len(b) for a, b in want[0].values()) > 3_000_000
    for coop in (0, 4096, None):
        got = run(coop, monkeypatch, recs, **RUNS[name])
        assert got[2] > 0, (name, coop)
        assert got[1] == want[1], (name, coop)
        for k in want[0]:
            assert got[0][k] == want[0][k], (name, coop, k)


@pytest.mark.parametrize("knobs", [{"PBSIM_COOP_DYNAMIC": "1"}, {"PBSIM_COOP_DYNAMIC": "0"}, {"PBSIM_COOP_WG": "1"}])
def test_state_limit_units_and_grid_change_nothing(knobs, monkeypatch):
    """units drawn from a counter or dealt round-robin, and one persistent workgroup for every unit of every class: the lane
    walker's bytes and statistics"""
    recs = records()
    for name in ("s31_default", "s50_default"):
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
        want = run(-1, monkeypatch, recs, **RUNS[name])
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        for coop in (0, 4096):
            got = run(coop, monkeypatch, recs, **RUNS[name])
            assert got[2] > 0 and got[:2] == want[:2], (name, coop, knobs)
