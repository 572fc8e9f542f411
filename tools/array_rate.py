"""Rate of the array output (pbsim_simulate_arrays) against the text left in HBM, on one synthetic record.

    python tools/array_rate.py [MBP] [DEPTH] [REPS]      (defaults: 100 Mbp x 20, 3 repetitions)

One record of MBP Mbp (tests/harness.py synth_bases_torch) x DEPTH, ERRHMM-ONT, the same seed for every path; each path
runs REPS times after one warm-up, a device synchronise around each run, and prints its best run:
  arrays+labels   simulate_arrays(labels=True)                  seq, qual, ref_pos: 6 B per base
  arrays          simulate_arrays(labels=False), no-op callback  seq, qual: 2 B per base
  text_hbm        simulate_wgs(collect=False)                   FASTQ + MAF text, left in HBM
For the array paths it also prints what the export moves: the scratch rows it reads (regions x MAF columns: the read row,
the reference row with labels) and the bytes it writes per base, and the same for the text path from its profile."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402  (before the library: see tests/conftest.py)

import harness  # noqa: E402
import pbsim3_amd as P  # noqa: E402


def main():
    mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 100
    depth = float(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    n = int(mbp * 1e6)
    ref = harness.synth_bases_torch(n, 5, device="cuda:0")
    torch.cuda.synchronize()
    p = P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, depth=depth, seed=17)
    ctx = P.Context(p, 0)
    ctx.load_errhmm(harness.model_path("ERRHMM-ONT.model"))
    ctx.set_reference_device(ref.data_ptr(), n, 1)
    seen = {}

    def labels_run():
        b = ctx.simulate_arrays(labels=True)
        seen["labels"] = (b.seq.numel(), b.offsets.numel() - 1, int((b.n_del.to(torch.int64)).sum()))

    def bare_run():
        got = []
        ctx.simulate_arrays(on_batch=lambda b: got.append((b.seq.numel(), b.offsets.numel() - 1)) or True, labels=False)
        seen["bare"] = (sum(g[0] for g in got), sum(g[1] for g in got))

    def text_run():
        ctx.prof_reset()
        ctx.simulate_wgs(collect=False)
        seen["text"] = ctx.prof_secondary()

    rows = {}
    for name, fn in (("arrays+labels", labels_run), ("arrays", bare_run), ("text_hbm", text_run)):
        best = None
        for r in range(reps + 1):
            P._check(ctx.lib.pbsim_device_synchronize(ctx.h))
            t0 = time.perf_counter()
            fn()
            P._check(ctx.lib.pbsim_device_synchronize(ctx.h))
            dt = time.perf_counter() - t0
            if r and (best is None or dt < best):
                best = dt
        bases = ctx.stats().res_len_total
        rows[name] = dict(seconds=round(best, 4), bases=bases, gbases_per_s=round(bases / best / 1e9, 2))
    bases, tasks, dels = seen["labels"]
    columns = bases + dels                      # MAF columns: a read base or a deletion each
    rows["arrays+labels"].update(read_bytes_per_base=round(2 * columns / bases, 3), write_bytes_per_base=6,
                                 task_bytes=49 * tasks)
    rows["arrays"].update(read_bytes_per_base=round(columns / bases, 3), write_bytes_per_base=2, task_bytes=49 * tasks)
    s = seen["text"]
    rows["text_hbm"].update(read_bytes_per_base=round(s["text_in"] / bases, 3),
                            write_bytes_per_base=round(s["text_out"] / bases, 3), text_ms=round(s["text_ms"], 2))
    print(json.dumps(dict(record_mbp=mbp, depth=depth, maf_columns=columns, tasks=tasks, paths=rows)))
    ctx.close()


if __name__ == "__main__":
    main()
