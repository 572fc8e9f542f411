// inflate.hip -- RFC 1951 inflate of BGZF members (SAMv1 4.1) on the GPU: the input-side counterpart of deflate.hip.
//
// A BGZF file is a gzip file cut into independent members of at most 64 KiB of output each; the host reads every member's
// compressed span (BSIZE) and output size (ISIZE) from the headers alone (inflate_host.cpp), so each member is decoded by
// its own workgroup straight into its final place.
//
//   layout  : one workgroup of one wave per member, grid-striding over the piece's members.  The decode state (bit buffer,
//             output position) is wave-uniform: every lane runs the same serial decode, and the lanes share the work that
//             is not serial -- the canonical code tables in LDS, match and stored-block copies (64 bytes per step), the
//             CRC-32 of the finished member.
//   input   : the member's compressed dwords sit across the wave, one per lane (a 256-byte window loaded in one coalesced
//             access); the bit buffer takes the next dword by readlane.  Only dwords that overlap the member's own span are
//             read, and bytes of them outside the span read as zero.
//   output  : written straight to its final offset in HBM (no 64 KiB LDS stage: that would cap a CU at two members in
//             flight, and a member's decode is latency-bound and serial -- the GPU's rate comes from many members at once).
//             A match reads back bytes the wave stored earlier; a workgroup-scope fence orders those stores before the
//             loads (one wave of one workgroup on one CU: it costs no wait there).  A match copy never depends on itself:
//             byte pos + i of a match at distance d is byte pos - d + (i mod d), already written before the match began.
//   checks  : codes 286-287 and distance codes 30-31, distances beyond the bytes produced, over-subscribed or incomplete
//             code sets (bar the single one-bit code RFC 1951 allows, and
//             a block without distance codes), stored LEN/NLEN, the member's span (truncated or
//             left over), ISIZE and CRC-32 -- each member leaves a status word (kernels.h InflateStatus), never a fault.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace pbsim {

namespace {

constexpr int kThreads = 64;      // one wave per member
constexpr int kFastBits = 9;      // first-level table: codes of up to 9 bits in one lookup
constexpr int kFast = 1 << kFastBits;
constexpr uint32_t kPoly = 0xEDB88320u;
constexpr int kCrcSeg = 1024;     // CRC bytes per lane: 64 x 1024 = the largest member
constexpr int kInflateBlocksMax = 16384;  // workgroups of a launch: beyond that they stride over the members

__constant__ uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                      31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                       193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// (the same product as deflate.hip's: a*b mod P, reflected -- bit 31 = x^0)
__device__ __forceinline__ uint32_t gf2_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}

// one canonical code in LDS: counts per length, the symbols sorted by (length, symbol), and the first-level table
struct Huff {
  uint32_t count[16];
  uint32_t next[16];       // scratch of the build: where the next symbol of each length goes
  uint16_t sym[288];
  uint16_t fast[kFast];    // next kFastBits bits (LSB first) -> sym | len << 9; 0: a longer code, or none
};

// the member's deflate bits: in[beg, end) of the piece; wave-uniform but for `win`
struct Bits {
  const uint32_t *in32;
  int64_t beg, end;
  int64_t wdw;     // dword index the window starts at (lane k holds dword wdw + k)
  uint32_t win;
  int64_t next;    // next dword to enter the bit buffer
  uint64_t bb;
  int bc;
  int lane;

  __device__ void load_window(int64_t d) {
    wdw = d;
    const int64_t dd = d + lane;
    uint32_t w = 0;
    if (dd * 4 < end && dd * 4 + 4 > beg) {
      w = in32[dd];
      const int64_t over = dd * 4 + 4 - end;  // bytes of this dword past the span
      if (over > 0) w &= 0xFFFFFFFFu >> (8 * over);
    }
    win = w;
  }
  __device__ uint32_t dword(int64_t d) {  // d never goes backwards between two start()s
    if (d - wdw >= kThreads) load_window(d);
    return (uint32_t)__builtin_amdgcn_readlane((int)win, (int)(d - wdw));
  }
  __device__ void start(int64_t byte) {  // read on from byte `byte` of the piece
    const int64_t d = byte >> 2;
    load_window(d);
    bb = dword(d) >> (8 * (byte & 3));
    bc = 32 - 8 * (int)(byte & 3);
    next = d + 1;
  }
  __device__ void need32() {
    if (bc < 32) {
      bb |= (uint64_t)dword(next++) << bc;
      bc += 32;
    }
  }
  __device__ uint32_t take(int n) {  // n <= 32, bc >= n
    const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1));
    bb >>= n;
    bc -= n;
    return v;
  }
  __device__ int64_t consumed() const { return (next * 4 - beg) * 8 - bc; }  // bits
};

// lens[0..n) -> h.  Returns 0 for a complete code, > 0 incomplete, < 0 over-subscribed; *max_len: the longest length used
__device__ int build(Huff &h, const uint8_t *lens, int n, int lane, int *max_len) {
  if (lane < 16) h.count[lane] = 0;
  __syncthreads();
  for (int i = lane; i < n; i += kThreads)
    if (lens[i]) atomicAdd(&h.count[lens[i]], 1u);
  __syncthreads();
  int left = 1, mx = 0, off = 0;
  for (int l = 1; l < 16; ++l) {
    const int c = (int)h.count[l];
    left = (left << 1) - c;
    if (c) mx = l;
    if (lane == l) h.next[l] = off;
    off += c;
  }
  *max_len = mx;
  if (left < 0) return left;
  __syncthreads();
  // symbols in order of (length, symbol): a chunk of 64 at a time, the rank within the chunk by ballot
  const uint64_t below = (1ull << lane) - 1;
  for (int c = 0; c < n; c += kThreads) {
    const int s = c + lane;
    const int l = s < n ? lens[s] : 0;
    int rank = 0, mine = 0;
    for (int k = 1; k < 16; ++k) {
      const uint64_t m = __ballot(l == k);
      if (l == k) rank = __popcll(m & below);
      if (lane == k) mine = __popcll(m);
    }
    if (l) h.sym[h.next[l] + rank] = (uint16_t)s;
    __syncthreads();
    if (lane > 0 && lane < 16) h.next[lane] += mine;
    __syncthreads();
  }
  // first-level table: entry e decoded canonically over its first kFastBits bits
  for (int e = lane; e < kFast; e += kThreads) {
    uint32_t v = 0;
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= kFastBits; ++l) {
      code |= (e >> (l - 1)) & 1;
      const int cnt = (int)h.count[l];
      if (code - first < cnt) {
        v = h.sym[index + code - first] | (uint32_t)l << 9;
        break;
      }
      index += cnt;
      first = (first + cnt) << 1;
      code <<= 1;
    }
    h.fast[e] = (uint16_t)v;
  }
  __syncthreads();
  return left;
}

// the next symbol of h, or -1 where no code of h matches
__device__ int decode(const Huff &h, Bits &b) {
  b.need32();
  const uint32_t e = h.fast[b.bb & (kFast - 1)];
  if (e) {
    b.take((int)(e >> 9));
    return (int)(e & 511u);
  }
  int code = 0, first = 0, index = 0;
  uint64_t bits = b.bb;
  for (int l = 1; l < 16; ++l) {
    code |= (int)(bits & 1);
    bits >>= 1;
    const int cnt = (int)h.count[l];
    if (code - first < cnt) {
      b.take(l);
      return h.sym[index + code - first];
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void k_inflate(const uint8_t *__restrict__ in, const InflateMember *__restrict__ members,
                                                      int64_t n_members, uint8_t *__restrict__ out, int32_t *__restrict__ status,
                                                      const uint32_t *__restrict__ crc_table, const uint32_t *__restrict__ pow128) {
  __shared__ uint32_t s_crc[1024];
  __shared__ Huff s_lit, s_dist;   // s_dist also holds the code-length code while a dynamic header is read
  __shared__ uint8_t s_lens[288 + 32];
  const int lane = threadIdx.x;
  for (int i = lane; i < 1024; i += kThreads) s_crc[i] = crc_table[i];
  __syncthreads();

  for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
    const InflateMember mb = members[m];
    uint8_t *const dst = out + mb.out_off;
    const int64_t isize = mb.out_len;
    const int64_t span_bits = (int64_t)mb.in_len * 8;
    Bits b;
    b.in32 = reinterpret_cast<const uint32_t *>(in);
    b.beg = mb.in_off;
    b.end = mb.in_off + mb.in_len;
    b.lane = lane;
    b.start(b.beg);
    int32_t st = kInfOk;
    int64_t pos = 0;
    bool last = false;
    while (!last && st == kInfOk) {
      b.need32();
      last = b.take(1) != 0;
      const uint32_t type = b.take(2);
      if (b.consumed() > span_bits) {
        st = kInfTruncated;
        break;
      }
      if (type == 0) {  // stored: LEN, NLEN on the next byte boundary, then LEN bytes
        b.take(b.bc & 7);
        b.need32();
        const uint32_t len = b.take(16), nlen = b.take(16);
        if (b.consumed() > span_bits) {
          st = kInfTruncated;
          break;
        }
        if (len != (~nlen & 0xFFFFu)) {
          st = kInfStoredLen;
          break;
        }
        const int64_t p = b.beg + b.consumed() / 8;
        if (p + len > b.end) {
          st = kInfTruncated;
          break;
        }
        if (pos + len > isize) {
          st = kInfLength;
          break;
        }
        for (uint32_t i = lane; i < len; i += kThreads) dst[pos + i] = in[p + i];
        pos += len;
        b.start(p + len);
        continue;
      }
      if (type == 3) {
        st = kInfBlockType;
        break;
      }
      int mx = 0;
      if (type == 1) {  // fixed codes (RFC 1951 3.2.6); distance codes 30-31 are in the code and refused when decoded
        for (int i = lane; i < 288 + 32; i += kThreads) s_lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
        __syncthreads();
        build(s_lit, s_lens, 288, lane, &mx);
        build(s_dist, s_lens + 288, 32, lane, &mx);
      } else {  // dynamic: HLIT, HDIST, HCLEN, the code-length code, the code lengths
        b.need32();
        const int hlit = (int)b.take(5) + 257, hdist = (int)b.take(5) + 1, hclen = (int)b.take(4) + 4;
        if (hlit > 286 || hdist > 30) {
          st = kInfTooMany;
          break;
        }
        uint64_t clbits = 0;  // 19 x 3 bits in kClOrder
        b.need32();
        for (int i = 0; i < hclen; ++i) {
          if (i == 10) b.need32();
          clbits |= (uint64_t)b.take(3) << (3 * i);
        }
        if (b.consumed() > span_bits) {
          st = kInfTruncated;
          break;
        }
        if (lane < 19) {
          int k = 0;
          while (kClOrder[k] != lane) ++k;
          s_lens[lane] = k < hclen ? (uint8_t)((clbits >> (3 * k)) & 7u) : 0;
        }
        __syncthreads();
        if (build(s_dist, s_lens, 19, lane, &mx) != 0) {  // the code-length code must be complete
          st = kInfClSet;
          break;
        }
        const int nlen = hlit + hdist;
        int i = 0;
        while (i < nlen) {
          const int sym = decode(s_dist, b);
          if (b.consumed() > span_bits) {
            st = kInfTruncated;
            break;
          }
          if (sym < 0) {
            st = kInfClSet;
            break;
          }
          if (sym < 16) {
            if (lane == 0) s_lens[i] = (uint8_t)sym;
            ++i;
            continue;
          }
          int rep, val = 0;
          if (sym == 16) {
            if (i == 0) {
              st = kInfRepeat;
              break;
            }
            __syncthreads();
            val = s_lens[i - 1];
            rep = 3 + (int)b.take(2);
          } else if (sym == 17) {
            rep = 3 + (int)b.take(3);
          } else {
            rep = 11 + (int)b.take(7);
          }
          if (i + rep > nlen) {
            st = kInfRepeat;
            break;
          }
          for (int j = lane; j < rep; j += kThreads) s_lens[i + j] = (uint8_t)val;
          i += rep;
        }
        if (st != kInfOk) break;
        __syncthreads();
        if (s_lens[256] == 0) {
          st = kInfNoEob;
          break;
        }
        // an incomplete set is refused unless it is one code of one bit, or -- distances only, as zlib -- no code at all
        // (a block of literals); a distance symbol of such a set is then refused where one is decoded
        int left = build(s_lit, s_lens, hlit, lane, &mx);
        if (left < 0 || (left > 0 && mx != 1)) {
          st = kInfLitSet;
          break;
        }
        left = build(s_dist, s_lens + hlit, hdist, lane, &mx);
        if (left < 0 || (left > 0 && mx > 1)) {
          st = kInfDistSet;
          break;
        }
      }
      // ---- the block's symbols
      for (;;) {
        int sym = decode(s_lit, b);
        if (b.consumed() > span_bits) {
          st = kInfTruncated;
          break;
        }
        if (sym < 0) {
          st = kInfLitCode;
          break;
        }
        if (sym < 256) {
          if (pos >= isize) {
            st = kInfLength;
            break;
          }
          if (lane == 0) dst[pos] = (uint8_t)sym;
          ++pos;
          continue;
        }
        if (sym == 256) break;
        sym -= 257;
        if (sym >= 29) {
          st = kInfLitCode;
          break;
        }
        b.need32();
        const int len = kLenBase[sym] + (int)b.take(kLenExtra[sym]);
        const int dsym = decode(s_dist, b);
        if (dsym < 0 || dsym >= 30) {
          st = b.consumed() > span_bits ? kInfTruncated : kInfDistCode;
          break;
        }
        b.need32();
        const int dist = kDistBase[dsym] + (int)b.take(kDistExtra[dsym]);
        if (b.consumed() > span_bits) {
          st = kInfTruncated;
          break;
        }
        if (dist > pos) {
          st = kInfTooFar;
          break;
        }
        if (pos + len > isize) {
          st = kInfLength;
          break;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the wave's earlier stores before these loads
        if (dist >= len) {
          if (lane < len) dst[pos + lane] = dst[pos - dist + lane];
          for (int i = lane + kThreads; i < len; i += kThreads) dst[pos + i] = dst[pos - dist + i];
        } else {
          for (int i = lane; i < len; i += kThreads) dst[pos + i] = dst[pos - dist + i % dist];
        }
        pos += len;
      }
    }
    if (st == kInfOk) {
      const int64_t used = b.consumed();
      if (used > span_bits) st = kInfTruncated;
      else if ((used + 7) / 8 < mb.in_len) st = kInfTrailing;
      else if (pos != isize) st = kInfLength;
    }
    __syncthreads();  // every store of the member before the CRC's loads
    if (st == kInfOk) {
      // lane t: bytes [isize - (64 - t) * 1024, isize - (63 - t) * 1024), the segments aligned to the member's end so that
      // the bytes after each one are a multiple of 128 (deflate_host_tables' pow128 steps)
      const int64_t seg_end = isize - (int64_t)(kThreads - 1 - lane) * kCrcSeg;
      const int64_t seg_beg = seg_end - kCrcSeg > 0 ? seg_end - kCrcSeg : 0;
      uint32_t c = 0;
      if (seg_end > seg_beg) {
        c = seg_beg == 0 ? 0xFFFFFFFFu : 0u;
        int64_t i = seg_beg;
        for (; i < seg_end && ((uintptr_t)(dst + i) & 3u); ++i) c = s_crc[(c ^ dst[i]) & 255u] ^ (c >> 8);
        for (; i + 4 <= seg_end; i += 4) {
          const uint32_t x = c ^ *reinterpret_cast<const uint32_t *>(dst + i);
          c = s_crc[768 + (x & 255u)] ^ s_crc[512 + ((x >> 8) & 255u)] ^ s_crc[256 + ((x >> 16) & 255u)] ^ s_crc[x >> 24];
        }
        for (; i < seg_end; ++i) c = s_crc[(c ^ dst[i]) & 255u] ^ (c >> 8);
        int k = (kThreads - 1 - lane) * (kCrcSeg / 128);  // 128-byte steps after the segment (<= 504)
        if (k > 255) {
          c = gf2_mul(c, pow128[255]);
          k -= 255;
        }
        c = gf2_mul(c, pow128[k]);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d, kThreads);
      const uint32_t crc = isize ? c ^ 0xFFFFFFFFu : 0u;
      if (crc != mb.crc) st = kInfCrc;
    }
    if (lane == 0) status[m] = st;
    __syncthreads();  // the tables and s_lens of this member are done with
  }
}

}  // namespace

const char *inflate_reason(int32_t s) {
  static const char *const kText[kInfCount] = {
      "ok",
      "invalid block type",
      "invalid stored block lengths",
      "too many length or distance symbols",
      "invalid code lengths set",
      "invalid bit length repeat",
      "invalid code -- missing end-of-block",
      "invalid literal/lengths set",
      "invalid distances set",
      "invalid literal/length code",
      "invalid distance code",
      "invalid distance too far back",
      "unexpected end of the deflate data",
      "the deflate data ends before the member's trailer",
      "incorrect data check",
      "incorrect length check",
  };
  return s >= 0 && s < kInfCount ? kText[s] : "unknown inflate status";
}

void launch_inflate(const uint8_t *in, const InflateMember *members, int64_t n_members, uint8_t *out, int32_t *status,
                    const uint32_t *d_crc_table, const uint32_t *d_pow128, hipStream_t s) {
  if (n_members <= 0) return;
  // enough workgroups to fill every CU many times over (a member's decode is one serial chain of dependent loads);
  // beyond that they stride, and the CRC tables are loaded once per workgroup
  const int64_t grid = n_members < kInflateBlocksMax ? n_members : kInflateBlocksMax;
  hipLaunchKernelGGL(k_inflate, dim3((unsigned)grid), dim3(kThreads), 0, s, in, members, n_members, out, status, d_crc_table,
                     d_pow128);
}

}  // namespace pbsim
