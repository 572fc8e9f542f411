"""pbsim_simulate_arrays without a GPU: the symbol is exported and bound, its refusals come before any device work, and the
test helper that derives the expected arrays from FASTQ + MAF text follows the rule of include/pbsim3_amd.h."""
import ctypes as C

import numpy as np

import maf_truth
import pbsim3_amd as P


def _sink(alloc=lambda *a: 1, on_batch=lambda *a: 1):
    return P.ArraySink(None, P.ARRAY_ALLOC_CB(alloc), P.ARRAY_BATCH_CB(on_batch))


def _refusal(params, sink):
    with P.Context(params, -1) as ctx:
        ok = ctx.lib.pbsim_simulate_arrays(ctx.h, C.byref(sink) if sink is not None else None)
        return ok, ctx.lib.pbsim_last_error().decode()


def test_simulate_arrays_is_exported_and_bound():
    lib = P.load()
    assert "pbsim_simulate_arrays" in [n for n, _, _ in P.API]
    fn = lib.pbsim_simulate_arrays
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.POINTER(P.ArraySink)]
    assert [f for f, _ in P.ReadArrays._fields_] == [f for f, _, _ in P.ARRAY_FIELDS]
    assert P.ReadBatch._fields == tuple(f for f, _, _ in P.ARRAY_FIELDS) + ("first_read",)
    assert callable(getattr(P.Context, "simulate_arrays", None))


def test_refuses_a_null_sink_and_null_callbacks():
    p = P.default_params()
    ok, msg = _refusal(p, None)
    assert ok == 0 and "sink" in msg, msg
    ok, msg = _refusal(p, P.ArraySink(None, P.ARRAY_ALLOC_CB(lambda *a: 1), P.ARRAY_BATCH_CB()))
    assert ok == 0 and "sink" in msg, msg
    ok, msg = _refusal(p, P.ArraySink(None, P.ARRAY_ALLOC_CB(), P.ARRAY_BATCH_CB(lambda *a: 1)))
    assert ok == 0 and "sink" in msg, msg


def test_refuses_the_sampling_method():
    ok, msg = _refusal(P.default_params(method=P.METHOD_SAMPLE), _sink())
    assert ok == 0 and "sampling method" in msg, msg


def test_without_a_device_fails_with_the_usual_message():
    for strategy in (P.STRATEGY_WGS, P.STRATEGY_TRANS, P.STRATEGY_TEMPL):
        ok, msg = _refusal(P.default_params(strategy=strategy), _sink())
        assert ok == 0 and "this context has no HIP device" in msg, msg


# A '+' block and a '-' block, each with one inserted base (reference '-') and one deleted base (read '-').
FASTQ = b"@S1_1\nACTGA\n+S1_1\n!!!!!\n@S1_2\nATGTC\n+S1_2\n#####\n"
MAF = (b"a\ns ref  10 5 + 100 AC-GTA\ns S1_1  0 5 + 5   ACTG-A\n\n"
       b"a\ns ref  20 5 + 100 G-CATT\ns S1_2  0 5 - 5   GACA-T\n\n")


def test_helper_on_a_hand_written_maf():
    e = maf_truth.expected_arrays(FASTQ, MAF, 1)
    assert bytes(e["seq"]) == b"ACTGAATGTC"
    assert e["qual"].tolist() == [0] * 5 + [2] * 5
    # '+': columns A/A C/C -/T G/G T/- A/A from 10; '-': read base i counts from the block's right end
    assert e["ref_pos"].tolist() == [10, 11, -1, 12, 14] + [24, 22, 21, -1, 20]
    assert e["offsets"].tolist() == [0, 5, 10]
    assert e["read_number"].tolist() == [1, 2]
    assert e["pass_index"].tolist() == [0, 0]
    assert e["strand"].tolist() == [0, 1]
    assert e["ref_start"].tolist() == [10, 20] and e["ref_span"].tolist() == [5, 5]
    assert e["maf_ins"].tolist() == [1, 1] and e["maf_del"].tolist() == [1, 1]
    assert e["ref_name"] == [b"ref", b"ref"]


def test_helper_reads_sam_records_and_names_with_spaces():
    sam = (b"@HD\tVN:1.5\n"
           b"S/1/0\t4\t*\t0\t255\t*\t*\t0\t0\tACG\t+,-\tcx:i:3\n"
           b"S/1/1\t4\t*\t0\t255\t*\t*\t0\t0\tCGT\t!!!\tcx:i:3\n")
    maf = (b"a\ns templ1 some text 0 3 + 3 ACG\ns S/1/0                0 3 + 3 ACG\n\n"
           b"a\ns templ1 some text 0 3 + 3 ACG\ns S/1/1                0 3 - 3 ACG\n\n")
    e = maf_truth.expected_arrays(sam, maf, 2)
    assert e["read_number"].tolist() == [1, 1] and e["pass_index"].tolist() == [0, 1]
    assert e["qual"].tolist() == [10, 11, 12, 0, 0, 0]
    assert e["ref_pos"].tolist() == [0, 1, 2, 2, 1, 0]
    assert e["ref_name"] == [b"templ1 some text"] * 2
    assert np.array_equal(e["offsets"], [0, 3, 6])
