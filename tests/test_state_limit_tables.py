"""CPU-side checks (no GPU) of the state-limit models (tests/golden/make_models.py): the class tables the product builds from
them reach exactly the designed states with the moduli the wave walkers need, the designed classes sit on both edges of every
chain count, and the golden cases of these models (tests/golden/cases.py STATE_LIMIT) give every designed class reads."""
import re

import numpy as np
import pytest

import harness
import pbsim3_amd as P
import product
from cases import CASES, STATE_LIMIT
from make_models import S31_DESIGN, S32_DESIGN, S50_DESIGN

ERR_DESIGN = {"SYNTH-ERRHMM-S31.model": S31_DESIGN, "SYNTH-ERRHMM-S32.model": S32_DESIGN}
DESIGN = dict(ERR_DESIGN, **{"SYNTH-QSHMM-S50.model": S50_DESIGN})


def err_chains(reach):
    """chains of eight start states coop_chain walks per lane (kernels.hip): two up to reach 15, three up to 23, four above"""
    return 2 if reach <= 15 else 3 if reach <= 23 else 4


def qs_chains(reach):
    """qcoop_walk_task's n_chains: start states 0 .. reach in chains of eight"""
    return (reach + 8) >> 3


def class_headers(model, method):
    """[(u32 header[16], class blob)] per accuracy class of the default accuracy range, from the product's host build"""
    ctx = P.Context(P.default_params(method=method), -1)
    (ctx.load_errhmm if method == P.METHOD_ERR else ctx.load_qshmm)(harness.model_path(model))
    blob = ctx.dump_table(2)
    p2a = np.frombuffer(ctx.dump_table(1), dtype=np.uint8)
    ctx.close()
    ncls = int(p2a[1:].max()) - int(p2a[1:].min()) + 1
    assert len(blob) % ncls == 0
    stride = len(blob) // ncls
    return [(np.frombuffer(blob[c * stride:c * stride + 64], dtype=np.uint32), blob[c * stride:(c + 1) * stride])
            for c in range(ncls)]


@pytest.mark.parametrize("model", sorted(ERR_DESIGN))
def test_errhmm_state_limit_reach_and_moduli(model):
    design = ERR_DESIGN[model]
    top = max(design.values())
    seen = {}
    for hdr, b in class_headers(model, P.METHOD_ERR):
        smax, init_rv, mode, acc, mc, reach = (int(hdr[i]) for i in (0, 1, 2, 4, 5, 6))
        assert smax == top and init_rv == 1000, (model, acc)
        rows = np.frombuffer(b[64:64 + 32 * (smax + 1)], dtype=np.uint16).reshape(smax + 1, 16)
        # every state up to the class's reach has a transition row ending at 1000; none beyond it has one
        assert all(int(rows[j][0]) == 1000 for j in range(1, reach + 1)), (model, acc)
        assert all(int(rows[j][0]) == 0 for j in range(reach + 1, smax + 1)), (model, acc)
        init_off = 64 + 48 * (smax + 1)
        assert int(np.frombuffer(b[init_off:init_off + 1000], dtype=np.uint8).max()) <= reach
        if mc in design:
            assert mode == 0 and reach == design[mc], (model, acc, reach, design[mc])
            seen[acc] = reach
    assert seen == design
    reaches = set(seen.values())
    # both edges of the three- and four-chain walks, the fourth chain's states 30 and 31, and classes far below smax
    assert {15, 16, 23, 24, 30, 31} <= reaches and min(reaches) == 1
    assert {err_chains(r) for r in reaches} == {2, 3, 4}
    # S31 is the largest model the ERRHMM wave walker takes; S32 is one state past it (kernels.h kCoopMaxStates)
    assert (top <= 31) == (product.NO_WAVE_MODELS.get(model) is None)


def test_qshmm_state_limit_reach_and_moduli():
    model = "SYNTH-QSHMM-S50.model"
    seen = {}
    for hdr, b in class_headers(model, P.METHOD_QS):
        smax, init_rv, has_model, acc, reach = (int(hdr[i]) for i in (0, 1, 2, 4, 6))
        assert smax == 50 and has_model == 1 and init_rv == 100, acc
        rv = np.frombuffer(b[64:64 + 4 * (smax + 1)], dtype=np.uint16).reshape(smax + 1, 2)
        # every reachable state's transition and emission moduli are 100 (QsClassTables::all_rv_100; the rows of states
        # beyond reach are empty and keep the reference's shared end_wk, pbsim.cpp:1974, whatever it was)
        assert all(int(rv[j][0]) == 100 and int(rv[j][1]) == 100 for j in range(1, reach + 1)), acc
        if acc in S50_DESIGN:
            assert reach == S50_DESIGN[acc], (acc, reach)
            seen[acc] = reach
    assert seen == S50_DESIGN
    # both edges of every chain count from one to seven: reach 8 k - 1 and 8 k
    chains = {}
    for r in seen.values():
        chains.setdefault(qs_chains(r), set()).add(r)
    assert sorted(chains) == [1, 2, 3, 4, 5, 6, 7]
    for n in range(1, 7):
        assert 8 * n - 1 in chains[n] and 8 * n in chains[n + 1]
    assert 50 in chains[7]


@pytest.mark.parametrize("case", sorted(STATE_LIMIT))
def test_state_limit_cases_give_every_designed_class_reads(case):
    """the expected number of reads of each designed class: the case's reads (depth x record length / the mean of the length
    table) times the class's share of the accuracy table (prob2acc, as the reference draws it) -- 20 or more"""
    argv = CASES[case]["args"]
    p, a = product.params_from_args(argv)
    ctx = P.Context(p, -1)
    p2l = np.frombuffer(ctx.dump_table(0), dtype=np.int32)[1:]
    p2a = np.frombuffer(ctx.dump_table(1), dtype=np.uint8)[1:]
    ctx.close()
    glen = int(re.fullmatch(r"INPUT:synth_(\d+)_\d+\.fa", a["--genome"]).group(1))
    reads = float(a["--depth"]) * glen / p2l.mean()
    share = np.bincount(p2a, minlength=101) / len(p2a)
    for acc in DESIGN[STATE_LIMIT[case]]:
        assert reads * share[acc] >= 20, (case, acc, reads * share[acc])
