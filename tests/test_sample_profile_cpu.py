"""The GPU profile builder's entry points (pbsim_sample_profile_from_bytes / _from_device, pbsim_load_sample_fastq,
pbsim_sample_profile_text, pbsim_set_sample_chunk_bytes; pbsim3_amd/csrc/sample_profile.cpp) where no device is needed:
they exist, they check their arguments first, and a tables-only context refuses them with its message and stays usable."""
import ctypes as C

import pytest

import pbsim3_amd as P

SYMBOLS = ["pbsim_sample_profile_from_bytes", "pbsim_sample_profile_from_device", "pbsim_load_sample_fastq",
           "pbsim_sample_profile_text", "pbsim_set_sample_chunk_bytes"]
FASTQ = b"@r\nACGT\n+\n" + b"5" * 200 + b"\n"


def params():
    return P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE)


def test_symbols_and_methods_exist():
    lib = P.load()
    bound = {n for n, _, _ in P.API}
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in bound, name
    for name in ("load_sample_fastq", "sample_profile_from_fastq", "sample_profile", "set_sample_chunk_bytes"):
        assert callable(getattr(P.Context, name)), name
    assert [f[0] for f in P.SampleStats._fields_] == [
        "num", "len_min", "len_max", "len_total", "num_filtered", "len_min_filtered", "len_max_filtered", "len_total_filtered",
        "len_mean_filtered", "len_sd_filtered", "accuracy_mean_filtered", "accuracy_sd_filtered"]
    assert C.sizeof(P.SampleStats) == 8 * 8 + 4 * 8


def test_tables_only_context_refuses_and_stays_usable(tmp_path):
    path = tmp_path / "s.fastq"
    path.write_bytes(FASTQ)
    with P.Context(params(), -1) as c:
        for call in (lambda: c.sample_profile_from_fastq(FASTQ), lambda: c.load_sample_fastq(str(path)), lambda: c.sample_profile(),
                     lambda: c.sample_profile_from_fastq(FASTQ)):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                call()
        st = P.SampleStats()
        assert c.lib.pbsim_sample_profile_from_device(c.h, C.c_void_p(16), 4, 0.75, 1.0, C.byref(st)) == 0
        assert b"no HIP device" in c.lib.pbsim_last_error()
        c.set_sample_chunk_bytes(1 << 20)         # needs no device
        c.set_sample_chunk_bytes(0)
        assert c.sam_header() is not None         # the context still answers


def test_argument_errors_come_first():
    with P.Context(params(), -1) as c:
        st = P.SampleStats()
        for fn, arg in ((c.lib.pbsim_sample_profile_from_bytes, FASTQ), (c.lib.pbsim_sample_profile_from_device, C.c_void_p(16))):
            assert fn(c.h, arg, -1, 0.75, 1.0, C.byref(st)) == 0                     # a negative size
            assert b"bad argument" in c.lib.pbsim_last_error()
            assert fn(c.h, None, 5, 0.75, 1.0, C.byref(st)) == 0                     # bytes promised, none given
            assert b"bad argument" in c.lib.pbsim_last_error()
            assert fn(c.h, arg, 4, 0.75, 1.0, None) == 0                             # nowhere to put the statistics
            assert b"bad argument" in c.lib.pbsim_last_error()
            assert fn(c.h, arg, 4, 0.9, 0.8, C.byref(st)) == 0
            assert b"accuracy_min exceeds accuracy_max" in c.lib.pbsim_last_error()
        with pytest.raises(P.PbsimError, match="accuracy_min exceeds accuracy_max"):
            c.sample_profile_from_fastq(FASTQ, 0.9, 0.8)
        with pytest.raises(P.PbsimError, match="accuracy_min exceeds accuracy_max"):
            c.load_sample_fastq("/nonexistent", 1.0, 0.5)
        with pytest.raises(P.PbsimError, match="bad argument"):
            c.set_sample_chunk_bytes(-1)
        n = C.c_int64(0)
        assert c.lib.pbsim_sample_profile_text(c.h, None, -1, C.byref(n)) == 0
        assert b"bad argument" in c.lib.pbsim_last_error()
        with pytest.raises(TypeError):
            c.sample_profile_from_fastq("not bytes")
