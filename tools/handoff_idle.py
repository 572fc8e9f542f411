#!/usr/bin/env python3
"""Where the link carries nothing at the edges of a job and between its rounds, from the stderr of one run with
PBSIM_TRACE=1 PBSIM_DEFLATE_TRACE=1 (e.g. `python bench.py --steps 2 2> trace.err`).

A lane call's [deflate] line carries the host time of its first copy's enqueue and of its last copy's completion; the job's
lines carry its entry and its return.  Per job this prints
  job entry -> first copy enqueued,
  for every round boundary: the last completion of round r (the later lane) -> the first enqueue of round r + 1 (the earlier lane),
  last completion -> return of pbsim_job_run.
The tail chains' calls (a few KB on lanes of their own) are left out.

usage: handoff_idle.py trace.err [label]"""
import re
import sys

CALL = re.compile(r"^\[deflate\] ([0-9.]+) MB -> ([0-9.]+) MB in .*first copy enqueued at ([0-9.]+), last copy complete at ([0-9.]+) ms(.*)$")
ENTER = re.compile(r"^\[pbsim job r0\] entered at ([0-9.]+) ms")
RET = re.compile(r"^\[pbsim job r0\] returns at ([0-9.]+) ms(.*)$")


def jobs(lines):
    cur = None
    for l in lines:
        m = ENTER.match(l)
        if m:
            cur = {"enter": float(m.group(1)), "calls": [], "ret": None, "note": ""}
            continue
        if cur is None:
            continue
        m = CALL.match(l)
        if m and "(chain lane)" not in m.group(5):
            cur["calls"].append((float(m.group(3)), float(m.group(4)), float(m.group(2)), "handed off" in m.group(5)))
            continue
        m = RET.match(l)
        if m:
            cur["ret"] = float(m.group(1))
            cur["note"] = m.group(2).lstrip("; ")
            yield cur
            cur = None


def rounds_of(calls):
    """lane calls -> rounds: the two lanes of a round overlap, rounds follow each other"""
    out = []
    for first, last, mb, handed in sorted(calls):
        if out and first < out[-1]["last"]:
            r = out[-1]
            r["last"] = max(r["last"], last)
            r["mb"] += mb
            r["handed"] += handed
        else:
            out.append({"first": first, "last": last, "mb": mb, "handed": int(handed)})
    return out


def main():
    path = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else path
    print("# idle link at the job's edges and round boundaries -- %s" % label)
    print("# (host clock; a boundary = last copy of round r complete, the later lane -> first copy of round r + 1 enqueued, the earlier lane)")
    for i, j in enumerate(jobs(open(path).read().splitlines())):
        rs = rounds_of(j["calls"])
        if not rs:
            continue
        gaps = [b["first"] - a["last"] for a, b in zip(rs, rs[1:])]
        busy = sum(r["last"] - r["first"] for r in rs)
        mb = sum(r["mb"] for r in rs)
        print("job %d: wall %.1f ms, %d rounds, %.1f MB of members%s" % (i, j["ret"] - j["enter"], len(rs), mb, ("; " + j["note"]) if j["note"] else ""))
        print("  job entry -> first copy      %8.2f ms" % (rs[0]["first"] - j["enter"]))
        print("  round boundaries (%2d)        %8.2f ms in all, mean %.2f, max %.2f" % (len(gaps), sum(gaps), sum(gaps) / max(1, len(gaps)), max(gaps or [0])))
        print("    each: " + " ".join("%.2f%s" % (g, "*" if b["handed"] else "") for g, b in zip(gaps, rs[1:])) + "   (*: the round's head was handed off)")
        print("  last copy -> return          %8.2f ms" % (j["ret"] - rs[-1]["last"]))
        print("  first copy -> last copy      %8.2f ms, of which inside rounds %.2f ms: %.1f GB/s over the rounds" % (rs[-1]["last"] - rs[0]["first"], busy, mb / busy if busy else 0))


if __name__ == "__main__":
    main()
