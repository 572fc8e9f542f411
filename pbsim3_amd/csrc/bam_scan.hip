// bam_scan.hip -- where the records of a BAM stream in HBM may start.  BAM records are chained by block_size, and a chain is
// serial.  Every BYTE position is tested instead, in parallel.  A workgroup stages a 4 KiB tile plus a 64-byte halo in LDS; a
// lane holds the 64 bytes around its sixteen positions in registers and takes the unaligned fields out of them with
// v_alignbyte.  Two passes (count, then write behind an exclusive scan of the tiles' counts) keep the hits in ascending order.
// What a position is tested against is the policy's (bam_scan.h); nothing else differs between the sort's scan and the
// sampling input's.  The hits are a superset of the record starts: the host walks the chain over them, and that walk alone
// decides (bam_chain.cpp).
#include "bam_scan.h"

#include "bam_fields.h"
#include "kernels.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
static_assert(kBamTile == kThreads * 16, "a lane tests sixteen positions");

// the 32-bit field at byte K of the lane's 64 bytes
template <int K>
__device__ __forceinline__ uint32_t field(const uint32_t (&w)[16]) {
  static_assert(K + 4 <= 64, "inside the lane's bytes");
  if constexpr ((K & 3) == 0) return w[K >> 2];
  else return __builtin_amdgcn_alignbyte(w[(K >> 2) + 1], w[K >> 2], (uint32_t)(K & 3));
}

// what every record's sizes satisfy, at position p = the lane's byte J: its block_size, or 0
template <int J>
__device__ __forceinline__ uint32_t sizes_fit(const uint32_t (&w)[16], const BamPacking &pk, int64_t p, int64_t lo, int64_t n) {
  const int32_t l_seq = (int32_t)field<J + kBamLSeq>(w);
  if (l_seq < 0) return 0;
  const uint32_t block_size = field<J>(w), l_read_name = field<J + kBamLReadName>(w) & 0xffu, n_cigar_op = field<J + kBamNCigarOp>(w) & 0xffffu;
  const int64_t need = 32 + (int64_t)l_read_name + 4 * (int64_t)n_cigar_op + ((int64_t)l_seq + 1) / 2 + l_seq;
  if ((int64_t)block_size < need || (int64_t)block_size > pk.max_block) return 0;
  if (p < lo || p + 4 + (int64_t)block_size > n) return 0;
  return block_size;
}

struct PlacedRecord {
  static constexpr BamPacking kPacking = kBamSortPacking;
  template <int J>
  static __device__ __forceinline__ uint32_t fits(const uint32_t (&w)[16], const uint8_t *, int64_t p, int64_t lo, int64_t n, int32_t n_ref) {
    // the twelve constant bytes first: nearly every position ends here
    if (field<J + kBamNextRefId>(w) != 0xffffffffu || field<J + kBamNextPos>(w) != 0xffffffffu || field<J + kBamTlen>(w) != 0u) return 0;
    const int32_t ref_id = (int32_t)field<J + kBamRefId>(w), pos = (int32_t)field<J + kBamPos>(w);
    if (ref_id < 0 || ref_id >= n_ref || pos < 0) return 0;
    return sizes_fit<J>(w, kPacking, p, lo, n);
  }
};

struct AnyRecord {
  static constexpr BamPacking kPacking = kBamSamplePacking;
  template <int J>
  static __device__ __forceinline__ uint32_t fits(const uint32_t (&w)[16], const uint8_t *buf, int64_t p, int64_t lo, int64_t n, int32_t n_ref) {
    const int32_t ref_id = (int32_t)field<J + kBamRefId>(w), next_ref_id = (int32_t)field<J + kBamNextRefId>(w);
    if (ref_id < -1 || ref_id >= n_ref || next_ref_id < -1 || next_ref_id >= n_ref) return 0;
    const int32_t pos = (int32_t)field<J + kBamPos>(w), next_pos = (int32_t)field<J + kBamNextPos>(w);
    if (pos < -1 || next_pos < -1) return 0;
    const uint32_t l_read_name = field<J + kBamLReadName>(w) & 0xffu;
    if (l_read_name == 0) return 0;
    const uint32_t block_size = sizes_fit<J>(w, kPacking, p, lo, n);
    // the one byte that is not in the lane's registers, for the few positions that come so far (inside the record: need <= block_size)
    if (block_size && buf[p + kBamFixed - 1 + l_read_name] != 0) return 0;
    return block_size;
  }
};

template <class Policy, int J>
__device__ __forceinline__ void fits_all(const uint32_t (&w)[16], const uint8_t *buf, int64_t p0, int64_t lo, int64_t n, int32_t n_ref,
                                         uint32_t (&size)[16], int &mine) {
  if constexpr (J < 16) {
    size[J] = Policy::template fits<J>(w, buf, p0 + J, lo, n, n_ref);
    mine += size[J] != 0;
    fits_all<Policy, J + 1>(w, buf, p0, lo, n, n_ref, size, mine);
  }
}

// kWrite false: tile_count[t - first_tile] = the hits of tile t (int64: the exclusive scan over them needs no conversion);
// true: the hits, packed, ascending, at out[tile_base[t - first_tile]..)
template <class Policy, bool kWrite>
__global__ __launch_bounds__(kThreads) void k_bam_scan(const uint8_t *buf, int64_t lo, int64_t n, int32_t n_ref, int64_t first_tile,
                                                      int64_t *tile_count, const int64_t *tile_base, uint64_t *out) {
  __shared__ uint4 sh[kThreads + 4];
  __shared__ int cnt[kThreads];
  const int i = threadIdx.x;
  const int64_t base = (first_tile + blockIdx.x) * kBamTile;
  const uint4 *g = reinterpret_cast<const uint4 *>(buf + base);  // (the buffer is aligned, and readable kBamSlack bytes past n)
  sh[i] = g[i];
  if (i < 4) sh[kThreads + i] = g[kThreads + i];
  __syncthreads();
  uint32_t w[16];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const uint4 x = sh[i + v];
    w[4 * v] = x.x;
    w[4 * v + 1] = x.y;
    w[4 * v + 2] = x.z;
    w[4 * v + 3] = x.w;
  }
  uint32_t size[16];
#pragma unroll
  for (int j = 0; j < 16; j++) size[j] = 0;
  int mine = 0;
  const int64_t p0 = base + 16 * i;
  if (p0 < n) fits_all<Policy, 0>(w, buf, p0, lo, n, n_ref, size, mine);  // (the fields of position 15 end at the lane's byte 50)
  const int total = __syncthreads_count(mine != 0);  // lanes with a hit
  if (!kWrite) {
    if (total == 0) {
      if (i == 0) tile_count[blockIdx.x] = 0;
      return;
    }
    cnt[i] = mine;
    __syncthreads();
    if (i == 0) {
      int64_t sum = 0;
      for (int k = 0; k < kThreads; k++) sum += cnt[k];
      tile_count[blockIdx.x] = sum;
    }
    return;
  }
  if (total == 0) return;
  cnt[i] = mine;
  __syncthreads();
  if (!mine) return;
  int64_t at = tile_base[blockIdx.x];
  for (int k = 0; k < i; k++) at += cnt[k];
#pragma unroll
  for (int j = 0; j < 16; j++)
    if (size[j]) out[at++] = Policy::kPacking.pack(p0 + j, size[j]);
}

template <class Policy>
void launch(const uint8_t *buf, int64_t lo, int64_t n, int32_t n_ref, int64_t first_tile, int64_t n_tiles, int64_t *tiles, uint64_t *out,
            hipStream_t s) {
  if (out) hipLaunchKernelGGL((k_bam_scan<Policy, true>), dim3((unsigned)n_tiles), dim3(kThreads), 0, s, buf, lo, n, n_ref, first_tile, nullptr, tiles, out);
  else hipLaunchKernelGGL((k_bam_scan<Policy, false>), dim3((unsigned)n_tiles), dim3(kThreads), 0, s, buf, lo, n, n_ref, first_tile, tiles, nullptr, out);
}

}  // namespace

hipError_t BamScan::need(DevBuf &b, size_t bytes, const char *what) {
  const hipError_t e = b.ensure(bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    oom_what = what;
    oom_bytes = bytes;
  }
  return e;
}

hipError_t BamScan::run(BamScanPolicy policy, const uint8_t *buf, int64_t lo, int64_t n, int32_t n_ref, hipStream_t s, std::vector<uint64_t> *hits) {
#define BAM_SCAN_OK(expr)                   \
  do {                                      \
    const hipError_t e_ = (expr);           \
    if (e_ != hipSuccess) return e_;        \
  } while (0)
  hits->clear();
  oom_what = nullptr;
  const int64_t first_tile = lo / kBamTile, n_tiles = (n + kBamTile - 1) / kBamTile - first_tile;
  if (n_tiles <= 0) return hipSuccess;
  auto pass = [&](uint64_t *out) {
    if (policy == kBamScanPlaced) launch<PlacedRecord>(buf, lo, n, n_ref, first_tile, n_tiles, d_tiles.as<int64_t>(), out, s);
    else launch<AnyRecord>(buf, lo, n, n_ref, first_tile, n_tiles, d_tiles.as<int64_t>(), out, s);
    return hipGetLastError();
  };
  BAM_SCAN_OK(need(d_tiles, (size_t)(n_tiles + 1) * 8, "the scan's tile counts"));
  BAM_SCAN_OK(need(d_scan_tmp, (size_t)(n_tiles / 1024 + 8) * 8, "the scan's scratch"));
  int64_t *d_total = d_tiles.as<int64_t>() + n_tiles, n_hits = 0;
  BAM_SCAN_OK(pass(nullptr));
  launch_exclusive_scan_i64(d_tiles.as<int64_t>(), d_tiles.as<int64_t>(), n_tiles, d_scan_tmp.as<int64_t>(), d_total, s);
  BAM_SCAN_OK(hipGetLastError());
  // (eight bytes into pageable memory: the sort makes a BamScan per call, and a pinned buffer for this one word would be
  // allocated and freed each time)
  BAM_SCAN_OK(hipMemcpyAsync(&n_hits, d_total, 8, hipMemcpyDeviceToHost, s));
  BAM_SCAN_OK(hipStreamSynchronize(s));
  if (n_hits <= 0) return hipSuccess;
  hits->resize((size_t)n_hits);
  BAM_SCAN_OK(need(d_hits, hits->size() * 8, "the candidate list"));
  BAM_SCAN_OK(pass(d_hits.as<uint64_t>()));
  BAM_SCAN_OK(hipMemcpyAsync(hits->data(), d_hits.p, hits->size() * 8, hipMemcpyDeviceToHost, s));
  return hipStreamSynchronize(s);
#undef BAM_SCAN_OK
}

}  // namespace pbsim
