"""bench.py --dump-outputs (bench_dump.py) on the CPU: streams of BGZF members made by zlib, handed over in pieces the way the
job's sinks receive them, come back as the head and tail of their TEXT, whatever the member and piece boundaries; and the
arguments that cannot be honoured are refused before anything touches a GPU."""
import ctypes
import os
import random
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import harness

sys.path.insert(0, harness.ROOT)
import bench_dump  # noqa: E402


def bgzf_member(text, level=6):
    """one BGZF member (SAMv1 4.1) of `text`, as the GPU's deflate frames them"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(text) + c.flush()
    hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(body) + 8 - 1)
    return hdr + body + struct.pack("<II", zlib.crc32(text), len(text))


def stream(text, member_text=32768, level=6, cuts=()):
    """the members of `text`: one per `member_text` bytes, and one more boundary at every offset in `cuts` (a round's end)"""
    bounds = sorted(set(list(range(0, len(text), member_text)) + [c for c in cuts if 0 < c < len(text)] + [len(text)]))
    return b"".join(bgzf_member(text[a:b], level) for a, b in zip(bounds, bounds[1:]))


def fastq_like(n, seed):
    rng = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n:
        L = rng.randint(50, 3000)
        seq = bytes(rng.choice(b"ACGT") for _ in range(L))
        qual = bytes(33 + rng.randint(0, 40) for _ in range(L))
        out += b"@S1_%d\n%s\n+S1_%d\n%s\n" % (i, seq, i, qual)
        i += 1
    return bytes(out[:n])


def feed(cap, which, rec, z, rng, shuffle=False):
    """hands `z` to the capture in pieces of random sizes, like the sink's callbacks; returns the buffers (kept alive)"""
    pieces, at = [], 0
    while at < len(z):
        n = min(len(z) - at, rng.randint(1, 400_000))
        pieces.append((at, ctypes.create_string_buffer(z[at:at + n], n)))
        at += n
    if shuffle:
        rng.shuffle(pieces)
    for off, buf in pieces:
        cap.put(which, rec, ctypes.addressof(buf), len(buf), off)
    return pieces


class FakeStats:
    def __init__(self, k):
        for i, f in enumerate(bench_dump.STATS_FIELDS):
            setattr(self, f, k * 100 + i + 0.5 * (i >= 8))


def test_head_and_tail_are_the_text_whatever_the_members(tmp_path):
    rng = random.Random(7)
    W = 20_000
    cap = bench_dump.OutputCapture(3, window=W)
    texts, keep = {}, []
    for rec in (1, 2, 3):
        read = fastq_like(300_000 if rec != 2 else 9_000, rec)     # record 2: shorter than a window
        maf = fastq_like(250_000, 10 + rec).replace(b"@", b"a ")
        texts[rec] = (read, maf)
        sizes = []
        for which, t in enumerate((read, maf)):
            z = stream(t, cuts=[rng.randrange(len(t)) for _ in range(5)])
            keep.append(feed(cap, which, rec, z, rng, shuffle=(rec == 3)))
            sizes.append(len(z))
        cap.done(rec, FakeStats(rec), *sizes)
    shapes = cap.write(str(tmp_path))
    assert shapes["stats"] == [3, len(bench_dump.STATS_FIELDS)]
    got = {n: np.load(os.path.join(str(tmp_path), n + ".npy")) for n in shapes}
    assert got["stats"].dtype == np.float64 and got["read_head"].dtype == np.float32
    assert got["stats"][1, 0] == 200.0 and got["stats"][2, 9] == 309.5
    for i, rec in enumerate((1, 2, 3)):
        for w, name in enumerate(("read", "maf")):
            t = texts[rec][w]
            head, tail = got[name + "_head"][i], got[name + "_tail"][i]
            n = min(W, len(t))
            assert bytes(head[:n].astype(np.uint8)) == t[:W], (rec, name)
            assert bytes(tail[:n].astype(np.uint8)) == t[-W:], (rec, name)
            assert (head[n:] == -1).all() and (tail[n:] == -1).all()


def test_tail_skips_a_header_look_alike_in_stored_members():
    """stored (level 0) members carry their text verbatim: a BGZF header inside the text must not be taken for a member start"""
    fake = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00\x10\x00"
    text = (fake + fastq_like(5000, 3)) * 40
    z = stream(text, member_text=4096, level=0)
    for cut in range(len(z) - 30000, len(z) - 20000, 997):
        assert bench_dump.tail_text(z[cut:], 8000, False) == text[-8000:]
    assert bench_dump.tail_text(z, 8000, True) == text[-8000:]
    assert bench_dump.head_text(z[:20000], 8000) == text[:8000]


def test_missing_tail_piece_is_an_error():
    cap = bench_dump.StreamCapture(1000)
    z = stream(fastq_like(200_000, 5))
    a = ctypes.create_string_buffer(z[:len(z) - 5000], len(z) - 5000)
    cap.put(ctypes.addressof(a), len(a), 0)
    with pytest.raises(ValueError):
        cap.texts(len(z), 1000)


def test_window_keeps_the_dump_under_the_limit():
    for n in (1, 4, 16, 1000):
        w = bench_dump.window_for(n)
        assert n * (4 * w * 4 + 8 * len(bench_dump.STATS_FIELDS)) <= bench_dump.LIMIT_BYTES
    assert bench_dump.window_for(4) == bench_dump.MAX_WINDOW


@pytest.mark.parametrize("args", [["--steps", "0"], ["--gpus", "2", "--dump-outputs", "x"], ["--replay-ranks", "8"],
                                  ["--gpus", "2", "--fresh-records"]])
def test_bench_refuses_before_touching_a_gpu(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(harness.ROOT, "bench.py")] + args, capture_output=True, text=True,
                       env=env, timeout=60)
    assert p.returncode != 0 and "bench.py:" in p.stderr
