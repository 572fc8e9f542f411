"""bench.py takes its model files from the committed gzip-compressed copies without writing into the tree (which may be
read-only to whoever runs the benchmark): the unpacked copy lies outside it and holds the committed bytes."""
import gzip
import os
import sys

import harness

sys.path.insert(0, harness.ROOT)
import bench  # noqa: E402


def test_model_files_are_unpacked_outside_the_tree():
    for name in ("ERRHMM-ONT.model", "QSHMM-RSII.model", "ERRHMM-SEQUEL.model"):
        p = bench.model_path(name)
        assert not os.path.realpath(p).startswith(os.path.realpath(harness.ROOT) + os.sep), p
        with gzip.open(os.path.join(harness.MODEL_GZ_DIR, name + ".gz"), "rb") as f:
            assert open(p, "rb").read() == f.read()
        assert bench.model_path(name) == p
