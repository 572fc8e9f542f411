"""bench_dump.py -- `bench.py --dump-outputs DIR`: what the timed path handed its caller in its last step, as .npy files.

A step of the headline job delivers ~55 GB of gzip members (FASTQ / BAM records and MAF, per record) plus every record's
statistics, so the dump is a fixed sample of it: the first and the last `window` bytes of every record's two streams as TEXT
(the members inflated), and the statistics in full.  The text is what the member boundaries do not change: a round's size
follows the free HBM, and so do where its members start and end, but never the bytes they inflate to.  The head covers the
first reads of a record, the tail its quota cut and truncated tail reads; the statistics count every read of the job.

Files (a stream shorter than `window` pads its row with -1):
  stats.npy                 float64 [records, len(STATS_FIELDS)]   pbsim_stats of every record, fields in STATS_FIELDS order
  read_head.npy, read_tail.npy, maf_head.npy, maf_tail.npy
                            float32 [records, window]              byte values 0..255 of the text

Capturing costs the last timed step a copy of the stream heads and of the last `2 * window + 128 KiB` bytes of the pieces
near a stream's end -- where the step before it (the same job) ended it, less 1 %; the members are inflated after the timed
region.  No GPU, no torch: tests/test_bench_dump.py feeds it BGZF members made by zlib."""
import ctypes
import os
import threading
import zlib

STATS_FIELDS = ("res_num", "res_pass_num", "res_len_total", "res_len_min", "res_len_max", "res_sub_num", "res_ins_num",
                "res_del_num", "res_depth", "res_len_mean", "res_len_sd", "res_accuracy_mean", "res_accuracy_sd",
                "res_sub_rate", "res_ins_rate", "res_del_rate")
STREAMS = ("read", "maf")
LIMIT_BYTES = 64 << 20       # everything the dump writes
MAX_WINDOW = 1 << 19


def window_for(n_records):
    """text bytes per head / tail window: four float32 windows per record stay within 3/4 of LIMIT_BYTES"""
    return max(4096, min(MAX_WINDOW, (LIMIT_BYTES * 3 // 4) // (16 * max(1, n_records))))


def _member_at(buf, i):
    """length of the BGZF member (SAMv1 4.1: gzip header with the 'BC' extra field) starting at buf[i], or 0"""
    if i + 18 > len(buf) or buf[i:i + 4] != b"\x1f\x8b\x08\x04" or buf[i + 10:i + 16] != b"\x06\x00BC\x02\x00":
        return 0
    return int.from_bytes(buf[i + 16:i + 18], "little") + 1


def inflate_members(buf):
    """the text of consecutive gzip members; a member cut off at the end yields the part of its text that is there"""
    out = bytearray()
    buf = bytes(buf)
    while buf:
        d = zlib.decompressobj(31)
        out += d.decompress(buf)
        if not d.eof:
            break
        buf = d.unused_data
    return bytes(out)


def head_text(buf, window):
    """text[:window] of a stream from its first compressed bytes"""
    return inflate_members(buf)[:window]


def tail_text(buf, window, whole):
    """text[-window:] of a stream from its LAST compressed bytes (`whole`: buf is the entire stream).  The first member
    inside the window is the first BGZF header from which whole members run exactly to the window's end."""
    start = 0 if whole else None
    i = 0
    while start is None:
        i = buf.find(b"\x1f\x8b\x08\x04", i)
        if i < 0:
            raise ValueError("no whole BGZF member in the last %d bytes of the stream" % len(buf))
        j = i
        while j < len(buf):
            n = _member_at(buf, j)
            if n == 0:
                break
            j += n
        if j == len(buf):
            start = i
        i += 1
    return inflate_members(buf[start:])[-window:]


class StreamCapture:
    """the head and the tail of one compressed stream, from pieces (offset, bytes) in any order.  `expected`: the stream's
    size in a previous run of the same job; only pieces that end within 1 % + tail_cap of it leave their tails here."""

    def __init__(self, window, expected=None):
        self.head_cap = 2 * window + (64 << 10)        # compressed bytes that inflate to at least `window` of text
        self.tail_cap = 2 * window + (128 << 10)
        self.tail_from = 0 if expected is None else int(expected * 0.99) - self.tail_cap
        self.head = bytearray()
        self.tails = []                                 # (offset, bytes): the last tail_cap bytes of the pieces near the end
        self.end = 0

    def put(self, ptr, n, off):
        if off < self.head_cap:
            k = min(n, self.head_cap - off)
            if len(self.head) < off + k:
                self.head.extend(bytes(off + k - len(self.head)))
            self.head[off:off + k] = ctypes.string_at(ptr, k)
        if off + n <= self.tail_from:
            return
        k = min(n, self.tail_cap)
        self.tails.append((off + n - k, ctypes.string_at(ptr + n - k, k)))
        self.end = max(self.end, off + n)
        lo = self.end - self.tail_cap
        if len(self.tails) > 8:
            self.tails = [t for t in self.tails if t[0] + len(t[1]) > lo]

    def texts(self, total, window):
        """(head text, tail text) of the stream of `total` compressed bytes"""
        if total == 0:
            return b"", b""
        lo = max(0, total - self.tail_cap)
        win = bytearray(total - lo)
        have = bytearray(total - lo)
        for off, data in self.tails:
            a, b = max(off, lo), min(off + len(data), total)
            if a < b:
                win[a - lo:b - lo] = data[a - off:b - off]
                have[a - lo:b - lo] = b"\x01" * (b - a)
        if have.count(0):
            raise ValueError("the last %d bytes of the stream did not all arrive (or it ended more than 1 %% before the "
                             "size it had in the run before)" % (total - lo))
        return head_text(self.head[:min(total, self.head_cap)], window), tail_text(bytes(win), window, lo == 0)


class OutputCapture:
    """What one run of the job delivers: per record, its two compressed streams (head / tail windows) and its statistics.
    put() is called from the sink's callbacks (the read and the MAF stream each from a thread of its own), done() once per
    record with the statistics and the streams' sizes.  `expect`: {record: (read bytes, MAF bytes)} of a previous run of the
    same job (CountingSink.stats), or None (every piece leaves its tail)."""

    def __init__(self, n_records, window=None, expect=None):
        self.window = window or window_for(n_records)
        self.expect = expect or {}
        self.streams = {}
        self.stats = {}
        self.sizes = {}
        self.lock = threading.Lock()

    def put(self, which, rec, ptr, n, off):
        with self.lock:
            sc = self.streams.get((which, rec))
            if sc is None:
                exp = self.expect.get(rec)
                sc = self.streams[(which, rec)] = StreamCapture(self.window, exp[which] if exp else None)
        sc.put(ptr, n, off)

    def done(self, rec, stats, read_bytes, maf_bytes):
        with self.lock:
            self.stats[rec] = [float(getattr(stats, f)) for f in STATS_FIELDS]
            self.sizes[rec] = (read_bytes, maf_bytes)

    def arrays(self):
        """{name: numpy array} of the dump"""
        import numpy as np
        recs = sorted(self.stats)
        out = {"stats": np.array([self.stats[r] for r in recs], dtype=np.float64).reshape(len(recs), len(STATS_FIELDS))}
        for w, name in enumerate(STREAMS):
            head = np.full((len(recs), self.window), -1, dtype=np.float32)
            tail = np.full((len(recs), self.window), -1, dtype=np.float32)
            for i, r in enumerate(recs):
                sc = self.streams.get((w, r))
                if sc is None:            # nothing delivered (text left in HBM): the row stays -1
                    continue
                h, t = sc.texts(self.sizes[r][w], self.window)
                head[i, :len(h)] = np.frombuffer(h, dtype=np.uint8)
                tail[i, :len(t)] = np.frombuffer(t, dtype=np.uint8)
            out[name + "_head"] = head
            out[name + "_tail"] = tail
        return out

    def write(self, directory):
        """writes DIR/<name>.npy; returns {name: shape}"""
        import numpy as np
        arrs = self.arrays()
        total = sum(a.nbytes for a in arrs.values())
        if total > LIMIT_BYTES:
            raise RuntimeError("output dump of %d bytes exceeds %d" % (total, LIMIT_BYTES))
        os.makedirs(directory, exist_ok=True)
        for name, a in arrs.items():
            np.save(os.path.join(directory, name + ".npy"), a)
        return {name: list(a.shape) for name, a in arrs.items()}
