#!/usr/bin/env python3
"""GPU time of one batch's truth + read emission in MAF mode beside aligned-BAM mode (pbsim_set_truth_bam): one batch
shaped like the headline's (ERRHMM-ONT, default lengths, `--reads` reads) walked and finalised through the batch
primitives, the emission timed by the engine's own HIP events (pbsim_prof_secondary; BAM mode includes the CIGAR count
pass in front of the sizes).  Prints one JSON line.

    python tools/truth_emit_time.py --model ERRHMM-ONT.model [--reads 850000] [--genome-mb 100] [--repeat 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True)
    ap.add_argument("--reads", type=int, default=850000)
    ap.add_argument("--genome-mb", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch
    import harness
    import pbsim3_amd as P
    model = a.model if os.path.exists(a.model) else harness.model_path(a.model)   # a bare name: the tests' committed copy
    n = a.genome_mb * 1000000
    ref = harness.synth_bases_torch(n, 5, device="cuda:0")
    torch.cuda.synchronize()
    p = P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, depth=1000.0, seed=1)
    out = {"reads": a.reads, "model": os.path.basename(a.model)}
    for mode in ("maf", "bam"):
        with P.Context(p, 0) as ctx:
            ctx.load_errhmm(model)
            ctx.set_scratch_bytes(int(a.reads * 2 * (2 * 9000 + 64) * 1.3) + (1 << 30))
            ctx.set_reference_device(ref.data_ptr(), n, 1)
            if mode == "bam":
                ctx.set_truth_bam(True)
            runs = []
            for k in range(a.repeat):
                ctx.prof_reset()
                before = ctx.prof_secondary()
                ctx.batch_walk(1 + k * a.reads, a.reads)
                bi = ctx.batch_finalize(0)
                ctx.lib.pbsim_device_synchronize(ctx.h)
                s = ctx.prof_secondary()
                ms = s["text_ms"] - before["text_ms"]
                runs.append(dict(ms=round(ms, 3), read_bytes=bi.read_text_bytes, truth_bytes=bi.maf_text_bytes, bases=bi.bases,
                                 maf_columns=bi.maf_columns,
                                 written_GBps=round((bi.read_text_bytes + bi.maf_text_bytes) / ms / 1e6, 1)))
            out[mode] = runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
