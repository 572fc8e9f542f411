#!/usr/bin/env python3
"""Generate tests/golden/model_fuzz.json by RUNNING THE REFERENCE ITSELF (oracle/_ref/pbsim_ref_philox, see make_golden.py)
on the generated models of tests/model_fuzz.py: per case and leg the sha256 of the model text and, per output file, the
length and the sha256.  Digests only: no model file and nothing of the reference is written into the tree.

A case the reference crashes on or does not finish lies outside model_fuzz.defined(): tighten the predicate there (with the
pbsim.cpp line in its comment) and run this again (under a time limit: such a model may send the reference round for
ever).  Run tests/test_model_fuzz_cpu.py's census first: it needs no digests.  Arguments: the cases to redo (default: all)."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import harness  # noqa: E402
import model_fuzz  # noqa: E402


def run_leg(case, leg):
    with tempfile.TemporaryDirectory() as td:
        args = model_fuzz.args_for(case, leg, model_fuzz.write_model(case, td))
        work = os.path.join(td, "work")
        os.makedirs(work)
        outs = harness.run_reference(args, "philox", work)
    return {k: {"sha256": harness.sha(v), "bytes": len(v)} for k, v in outs.items()}


def main():
    only = sys.argv[1:]
    path = os.path.join(HERE, "model_fuzz.json")
    out = json.load(open(path)) if only and os.path.exists(path) else {}
    for case in model_fuzz.CASES:
        if only and case not in only:
            continue
        for leg in model_fuzz.CASES[case]["legs"]:
            entry = {"model_sha256": model_fuzz.model_sha(model_fuzz.model_of(case)[0]), "outputs": run_leg(case, leg)}
            out[f"{case}/{leg}"] = entry
            print(case, leg, {k: e["bytes"] for k, e in entry["outputs"].items()}, flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
