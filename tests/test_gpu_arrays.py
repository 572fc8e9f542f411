"""pbsim_simulate_arrays on the GPU: for every wgs / trans / templ golden case the arrays equal what tests/maf_truth.py derives
from the text the same inputs and seed give (the text itself pinned to the reference's digests first), the statistics equal
the text run's, batching and labels change nothing, no text kernel runs, refused batches leave the context usable, and a
record of more than a Gbase agrees with its text."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import harness
import maf_truth
import pbsim3_amd as P
import product
from cases import CASES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MANIFEST = harness.load_manifest()
ARRAY_CASES = sorted(c for c in CASES if "sample" not in c)
META = ("read_number", "pass_index", "strand", "ref_start", "ref_span")


def _model(ctx, p, a):
    if p.method == P.METHOD_ERR:
        ctx.load_errhmm(a["--errhmm"])
    else:
        ctx.load_qshmm(a["--qshmm"])


def _units(case):
    """[(loader, label)] of a case: wgs -> its records (set_reference + census); trans/templ -> the unit file.  A
    loader takes a fresh-or-reused context and prepares its next unit."""
    args = harness.resolve(CASES[case]["args"])
    p, a = product.params_from_args(args)
    if p.strategy == P.STRATEGY_WGS:
        recs = product.read_fasta(a["--genome"])

        def census(ctx):
            if p.hp_del_bias != 1:
                for r in recs:
                    ctx.add_hp_census(r)
                ctx.finish_hp_census()
        return p, a, [(lambda ctx, r=r, i=i: ctx.set_reference(r, i), i, r) for i, r in enumerate(recs, 1)], census
    if p.strategy == P.STRATEGY_TRANS:
        return p, a, [(lambda ctx: ctx.load_transcript_file(a["--transcript"]), None, None)], lambda ctx: None
    return p, a, [(lambda ctx: ctx.load_template_file(a["--template"]), None, None)], lambda ctx: None


def _unit_names(p, a):
    if p.strategy == P.STRATEGY_TRANS:
        with open(a["--transcript"], "rb") as f:
            return [ln.split(b"\t", 1)[0][:128] for ln in f.read().split(b"\n") if ln.strip()]
    with open(a["--template"], "rb") as f:
        return [ln[1:].rstrip(b"\r")[:128] for ln in f.read().split(b"\n") if ln.startswith(b">")]


def _stats(s):
    return {f: getattr(s, f) for f, _ in P.Stats._fields_}


def _same_stats(x, y, what):
    for k in x:
        a, b = x[k], y[k]
        assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), (what, k, a, b)


def _np(batch):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in batch._asdict().items() if k != "first_read"}


def text_runs(case, scratch_mb=None):
    """[(read text, MAF text, stats)] per unit, through the text drivers; the text equals the reference's goldens"""
    p, a, units, census = _units(case)
    gold = MANIFEST[f"{case}/philox"]
    out = []
    with P.Context(p, 0) as ctx:
        if scratch_mb:
            ctx.set_scratch_bytes(scratch_mb << 20)
        _model(ctx, p, a)
        census(ctx)
        for load, rec, _ in units:
            load(ctx)
            rt, mt = ctx.simulate_wgs() if rec else ctx.simulate_trans()
            if p.pass_num > 1:
                rt = ctx.sam_header() + rt
            name = ("_%04d" % rec if rec else "") + (".fq" if p.pass_num == 1 else ".sam")
            maf = ("_%04d" % rec if rec else "") + ".maf"
            assert harness.sha(rt) == gold[name]["sha256"], (case, name)
            assert harness.sha(mt) == gold[maf]["sha256"], (case, maf)
            out.append((rt, mt, _stats(ctx.stats())))
    return out


def array_runs(case, scratch_mb=None, labels=True):
    """[(ReadBatch as numpy, stats)] per unit, through pbsim_simulate_arrays on a fresh context"""
    p, a, units, census = _units(case)
    out = []
    with P.Context(p, 0) as ctx:
        if scratch_mb:
            ctx.set_scratch_bytes(scratch_mb << 20)
        _model(ctx, p, a)
        census(ctx)
        for load, _, _ in units:
            load(ctx)
            b = ctx.simulate_arrays(labels=labels)
            out.append((_np(b), _stats(ctx.stats())))
    return out


def check_against_text(case, arrays, texts):
    p, a, units, _ = _units(case)
    names = None if p.strategy == P.STRATEGY_WGS else _unit_names(p, a)
    for (got, st_arr), (rt, mt, st_txt), (_, rec, _) in zip(arrays, texts, units):
        e = maf_truth.expected_arrays(rt, mt, p.pass_num)
        for k in ("seq", "qual", "ref_pos", "offsets") + META:
            assert got[k].dtype == e[k].dtype, (case, k, got[k].dtype)
            if not np.array_equal(got[k], e[k]):
                bad = np.flatnonzero(got[k] != e[k]) if got[k].shape == e[k].shape else [None]
                raise AssertionError(f"{case} unit {rec}: {k} differs ({got[k].shape} vs {e[k].shape}, first at {bad[0]})")
        assert np.array_equal(got["n_ins"], e["maf_ins"]) and np.array_equal(got["n_del"], e["maf_del"]), case
        if rec:
            assert (got["unit"] == rec).all(), case
        else:
            assert [names[u] for u in got["unit"]] == e["ref_name"], case
            assert (np.diff(got["unit"]) >= 0).all(), case     # reads are dealt to the units in load order
        assert int(got["n_sub"].sum()) == st_arr["res_sub_num"], case
        assert int(got["n_ins"].sum()) == st_arr["res_ins_num"], case
        assert int(got["n_del"].sum()) == st_arr["res_del_num"], case
        _same_stats(st_arr, st_txt, case)


@pytest.mark.parametrize("case", ARRAY_CASES)
def test_arrays_match_the_text_of_every_golden_case(case):
    check_against_text(case, array_runs(case), text_runs(case))


BATCH_CASES = ["wgs_errhmm_sequel_pass3", "wgs_qshmm_rsii_pass1", "trans_qshmm_rsii", "templ_errhmm_rsii_pass3_hpbias2"]


@pytest.mark.parametrize("case", BATCH_CASES)
def test_batching_and_labels_change_nothing(case):
    whole = array_runs(case)
    many = array_runs(case, scratch_mb=4)
    bare = array_runs(case, labels=False)
    for (x, sx), (y, sy), (z, sz) in zip(whole, many, bare):
        for k in x:
            assert np.array_equal(x[k], y[k]), (case, k)
            if k != "ref_pos":
                assert np.array_equal(x[k], z[k]), (case, k)
        assert z["ref_pos"] is None
        _same_stats(sx, sy, case)
        _same_stats(sx, sz, case)


def test_no_text_or_deflate_kernel_runs():
    case = "wgs_errhmm_sequel_pass3"
    seen = []
    p, a, units, census = _units(case)
    with P.Context(p, 0) as ctx:
        _model(ctx, p, a)
        ctx.set_deflate(3)
        for load, _, _ in units:
            load(ctx)
            ctx.prof_reset()
            b = ctx.simulate_arrays()
            assert b.seq.numel() > 0
            s = ctx.prof_secondary()
            seen.append((s["text_launches"], s["deflate_launches"]))
    assert seen and all(x == (0, 0) for x in seen), seen


# ---- refusals: a raw pbsim_array_sink whose alloc hands over what the test chooses
def _raw_run(ctx, make, on_batch=lambda *a: 1):
    keep = []

    def alloc(user, tasks, bases, out):
        t = make(tasks, bases)
        if t is None:
            return 0
        keep.append(t)
        for name, x in t.items():
            setattr(out.contents, name, x.data_ptr() or None)
        return 1

    sink = P.ArraySink(None, P.ARRAY_ALLOC_CB(alloc), P.ARRAY_BATCH_CB(on_batch))
    ok = ctx.lib.pbsim_simulate_arrays(ctx.h, C.byref(sink))
    return ok, ctx.lib.pbsim_last_error().decode()


def _tensors(tasks, bases, device):
    t = {}
    for name, dtype, per in P.ARRAY_FIELDS:
        n = bases if per == "base" else tasks + 1 if per == "offset" else tasks
        t[name] = torch.empty(n, dtype=getattr(torch, dtype), device=device)
    return t


def test_refused_batches_leave_the_context_usable():
    case = "wgs_errhmm_sequel_pass3"
    texts = text_runs(case, scratch_mb=4)
    p, a, units, census = _units(case)
    load = units[0][0]
    with P.Context(p, 0) as ctx:
        ctx.set_scratch_bytes(4 << 20)      # several batches per record
        _model(ctx, p, a)
        load(ctx)

        def again():
            b = _np(ctx.simulate_arrays())
            check_against_text(case, [(b, _stats(ctx.stats()))], texts[:1])

        ok, msg = _raw_run(ctx, lambda tasks, bases: None)
        assert ok == 0 and "alloc" in msg, msg
        again()
        calls = []

        def stop_second(batch):
            calls.append(batch.first_read)
            return len(calls) < 2
        with pytest.raises(P.PbsimError, match="on_batch"):
            ctx.simulate_arrays(on_batch=stop_second)
        assert len(calls) == 2
        again()
        ok, msg = _raw_run(ctx, lambda tasks, bases: _tensors(tasks, bases, "cpu"))
        assert ok == 0 and "seq" in msg, msg
        again()
        if torch.cuda.device_count() > 1:
            ok, msg = _raw_run(ctx, lambda tasks, bases: _tensors(tasks, bases, "cuda:1"))
            assert ok == 0 and "not device memory of device 0" in msg, msg
            again()


def test_arrays_agree_with_the_text_of_a_gigabase_record():
    """one synthetic record of 50 Mbp x depth 20 (ERRHMM-ONT): seq, qual and ref_pos of the array path equal what the
    FASTQ + MAF text of the same record gives (the text parsed on the GPU)"""
    n, depth, seed = 50_000_000, 20, 17
    p = P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, depth=depth, seed=seed)
    ref = harness.synth_bases_torch(n, 5, device="cuda:0")
    torch.cuda.synchronize()

    def run(fn):
        with P.Context(p, 0) as ctx:
            ctx.load_errhmm(harness.model_path("ERRHMM-ONT.model"))
            ctx.set_reference_device(ref.data_ptr(), n, 1)
            return fn(ctx)
    batch = run(lambda ctx: ctx.simulate_arrays())
    assert batch.seq.numel() >= 1_000_000_000
    rt, mt = run(lambda ctx: ctx.simulate_wgs())
    dev = batch.seq.device
    # FASTQ: line 4 k + 1 is a read's sequence, 4 k + 3 its qualities
    t = torch.frombuffer(bytearray(rt), dtype=torch.uint8).to(dev)
    del rt
    nl = t == 10
    line = torch.cumsum(nl, 0) - nl.to(torch.int64)
    keep = ~nl
    assert torch.equal(t[keep & (line % 4 == 1)], batch.seq)
    assert torch.equal(t[keep & (line % 4 == 3)] - 33, batch.qual)
    del t, nl, line, keep
    # MAF: per block "a", the reference line, the read line, an empty line; a row is the text behind a line's last space
    heads = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(rb"\ns ref +(\d+) +(\d+) \+", mt)]
    strands = [m.group(1) == b"-" for m in re.finditer(rb" ([+-]) +\d+ [^ \n]+\n\n", mt)]
    assert len(heads) == len(strands) == batch.offsets.numel() - 1
    m = torch.frombuffer(bytearray(mt), dtype=torch.uint8).to(dev)
    del mt
    nl = m == 10
    line = torch.cumsum(nl, 0) - nl.to(torch.int64)
    n_lines = int(line[-1]) + 1
    pos = torch.arange(m.numel(), device=dev)
    last_sp = torch.full((n_lines,), -1, dtype=torch.int64, device=dev)
    sp = m == 32
    last_sp.scatter_reduce_(0, line[sp], pos[sp], reduce="amax")
    row = (~nl) & (pos > last_sp[line])
    kind = line % 4
    ref_row, read_row = m[row & (kind == 1)], m[row & (kind == 2)]
    block = (line[row & (kind == 1)] // 4)
    del m, nl, line, pos, sp, row, kind
    assert ref_row.numel() == read_row.numel()
    start = torch.tensor([h[0] for h in heads], dtype=torch.int64, device=dev)
    minus = torch.tensor(strands, dtype=torch.bool, device=dev)
    ref_ok, read_ok = ref_row != 45, read_row != 45

    def within_block(x):      # exclusive count of x in front of each column, inside its block
        c = torch.cumsum(x.to(torch.int64), 0) - x.to(torch.int64)
        first = torch.searchsorted(block, torch.arange(start.numel(), device=dev))
        return c - c[first][block]
    col_ref = start[block] + within_block(ref_ok)
    k = within_block(read_ok)
    q = torch.zeros(start.numel(), dtype=torch.int64, device=dev).index_add_(0, block, read_ok.to(torch.int64))
    first_base = torch.cumsum(q, 0) - q
    i = torch.where(minus[block], q[block] - 1 - k, k) + first_base[block]
    want = torch.empty_like(batch.ref_pos)
    want[i[read_ok]] = torch.where(ref_ok, col_ref, -1)[read_ok].to(torch.int32)
    assert torch.equal(want, batch.ref_pos)
