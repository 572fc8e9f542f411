// bam_eval.hip -- the kernels of pbsim_truth_bam_eval: a mapper's BAM scored against the truth BAMs, all of them inflated in HBM
// and their records located (bam_scan.hip, bam_chain.cpp).
//
//   keys       : one lane per record: the hash of the read name, the address, pos + the reference span of the CIGAR.  A record
//                of more than 64 ops (the truth's 65 535-op records, a CG placeholder's neighbours) is summed by its whole
//                wave, op k by lane k mod 64, so that it does not hold one lane for thousands of loads.
//   sort       : rocPRIM's radix sort of the truth's (hash, record number) pairs (bam_sort.hip's bs_sort_pairs).
//   duplicates : one lane per place of the sorted order walks back over the places of equal hash and compares the name bytes:
//                with all 64 bits a run is one place long; with hash_bits of a test it costs the square of the run.
//   join       : one lane per query record; a primary searches its hash among the sorted keys, walks the run of equal hashes
//                comparing the NAME BYTES, and puts its record number into the truth record's slot with atomicMin: the
//                smallest number is the smallest inflated offset.
//   verdict    : one lane per truth record applies the rule (include/pbsim3_amd.h) to the record in its slot; counts and the
//                MAPQ histogram are added up per workgroup in LDS and flushed with one vector atomic per cell that is not 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bam_eval.h"
#include "bam_fields.h"
#include "device_util.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;

// MIDNSHP=X: M 0, D 2, N 3, = 7, X 8 consume the reference
__device__ __forceinline__ int64_t ref_len(uint32_t v) { return (0x18du >> (v & 15u)) & 1u ? (int64_t)(v >> 4) : 0; }

__device__ __forceinline__ uint32_t name_len(const uint8_t *p) {
  const uint32_t l = p[kBamLReadName];
  return l ? l - 1 : 0;
}

// FNV-1a over the bytes, then the finaliser of MurmurHash3: every bit of the result depends on every byte
__device__ __forceinline__ uint64_t hash_name(const uint8_t *name, uint32_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t k = 0; k < n; k++) h = (h ^ name[k]) * 0x100000001b3ull;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

__device__ __forceinline__ bool same_name(const uint8_t *a, const uint8_t *b) {
  const uint32_t n = name_len(a);
  if (n != name_len(b)) return false;
  for (uint32_t k = 0; k < n; k++)
    if (a[kBamFixed + k] != b[kBamFixed + k]) return false;
  return true;
}

__global__ __launch_bounds__(kThreads) void k_eval_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, int size_bits,
                                                       uint64_t hash_mask, const int32_t *ref_map, int64_t first, uint64_t *ptr,
                                                       uint64_t *hash, int64_t *end, int32_t *gref, uint32_t *idx) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = r < n_rec;  // (no early return: the wave path below needs every lane)
  const uint8_t *p = stream;
  int64_t cig = 0, span = 0;
  uint32_t n_ops = 0;
  uint64_t h = 0;
  if (live) {
    p = stream + (int64_t)(rec[r] >> size_bits);
    const uint32_t l_read_name = p[kBamLReadName];
    n_ops = ld16(p + kBamNCigarOp);
    h = hash_name(p + kBamFixed, name_len(p)) & hash_mask;
    cig = (int64_t)(p + kBamFixed + l_read_name);
    if (n_ops <= 64)
      for (uint32_t k = 0; k < n_ops; k++) span += ref_len(ld32((const uint8_t *)cig + 4 * k));
  }
  // the records of more than 64 ops, one after the other, each by the whole wave
  for (uint64_t big = __ballot(live && n_ops > 64); big; big &= big - 1) {
    const int src = __ffsll((long long)big) - 1;
    const uint8_t *c = (const uint8_t *)__shfl(cig, src, 64);
    const uint32_t n = __shfl(n_ops, src, 64);
    int64_t part = 0;
    for (uint32_t k = lane; k < n; k += 64) part += ref_len(ld32(c + 4 * (int64_t)k));
    for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
    if (lane == src) span = part;
  }
  if (!live) return;
  const int64_t at = first + r;
  ptr[at] = (uint64_t)p;
  hash[at] = h;
  end[at] = (int64_t)(int32_t)ld32(p + kBamPos) + (span > 0 ? span : 1);
  if (ref_map) {  // (the truth: the locator has checked 0 <= refID < n_ref)
    gref[at] = ref_map[(int32_t)ld32(p + kBamRefId)];
    idx[at] = (uint32_t)at;
  }
}

__global__ __launch_bounds__(kThreads) void k_eval_duplicates(const uint64_t *key, const uint32_t *perm, const uint64_t *t_ptr,
                                                             int64_t n_truth, unsigned long long *dup) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < 1 || i >= n_truth) return;
  const uint64_t k = key[i];
  if (key[i - 1] != k) return;
  const uint32_t mine = perm[i];
  const uint8_t *a = (const uint8_t *)t_ptr[mine];
  for (int64_t j = i - 1; j >= 0 && key[j] == k; j--) {
    const uint32_t other = perm[j];
    if (!same_name(a, (const uint8_t *)t_ptr[other])) continue;
    const uint32_t later = max(mine, other), earlier = min(mine, other);
    atomicMin(dup, (unsigned long long)later << 32 | earlier);
  }
}

__global__ __launch_bounds__(kThreads) void k_eval_join(const uint64_t *q_ptr, const uint64_t *q_hash, int64_t n_query, const uint64_t *key,
                                                       const uint32_t *perm, const uint64_t *t_ptr, int64_t n_truth, uint32_t *first,
                                                       unsigned long long *cls) {
  __shared__ unsigned int sh[5];  // primary, secondary, supplementary, unknown, known
  if (threadIdx.x < 5) sh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q < n_query) {
    const uint8_t *p = (const uint8_t *)q_ptr[q];
    const uint32_t flag = ld16(p + kBamFlag);
    if (flag & 0x100u) {
      atomicAdd(&sh[1], 1u);
    } else if (flag & 0x800u) {
      atomicAdd(&sh[2], 1u);
    } else {
      atomicAdd(&sh[0], 1u);
      const uint64_t h = q_hash[q];
      int64_t lo = 0, hi = n_truth;  // the first place with key >= h
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key[mid] < h) lo = mid + 1;
        else hi = mid;
      }
      bool known = false;
      for (int64_t j = lo; j < n_truth && key[j] == h; j++) {
        const uint32_t t = perm[j];
        if (!same_name(p, (const uint8_t *)t_ptr[t])) continue;
        atomicMin(&first[t], (uint32_t)q);
        known = true;
        break;  // (a name is in the truth once)
      }
      atomicAdd(&sh[known ? 4 : 3], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < 5 && sh[threadIdx.x]) atomicAdd(&cls[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void k_eval_verdict(const uint64_t *t_ptr, const int64_t *t_end, const int32_t *t_gref,
                                                          const uint32_t *first, int64_t n_truth, const uint64_t *q_ptr, const int64_t *q_end,
                                                          const int32_t *query_map, int32_t n_query_ref, int32_t permille, uint8_t *verdict,
                                                          unsigned long long *res, unsigned long long *hist) {
  __shared__ unsigned int sh[512 + 4];  // the histogram, then missing, unmapped, correct, wrong: at most kThreads each
  for (int k = threadIdx.x; k < 512 + 4; k += kThreads) sh[k] = 0;
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t < n_truth) {
    const uint32_t q = first[t];
    uint8_t v;
    if (q == kEvalNoRecord) {
      v = 0;
    } else {
      const uint8_t *qp = (const uint8_t *)q_ptr[q];
      const uint32_t q_flag = ld16(qp + kBamFlag);
      const int32_t q_ref = (int32_t)ld32(qp + kBamRefId);
      if ((q_flag & 4u) || q_ref < 0) {
        v = 1;
      } else {
        const uint8_t *tp = (const uint8_t *)t_ptr[t];
        const int64_t ts = (int32_t)ld32(tp + kBamPos), te = t_end[t], qs = (int32_t)ld32(qp + kBamPos), qe = q_end[q];
        const int64_t inter = min(te, qe) - max(ts, qs), uni = max(te, qe) - min(ts, qs);
        const int32_t q_gref = q_ref < n_query_ref ? query_map[q_ref] : -1;
        const bool good = q_gref == t_gref[t] && ((q_flag ^ ld16(tp + kBamFlag)) & 16u) == 0 && inter > 0 &&
                          inter * 1000 >= (int64_t)permille * uni;
        v = good ? 3 : 2;
        const uint32_t mapq = qp[kBamLReadName + 1];
        atomicAdd(&sh[2 * mapq], 1u);
        if (!good) atomicAdd(&sh[2 * mapq + 1], 1u);
      }
    }
    verdict[t] = v;
    atomicAdd(&sh[512 + (v == 0 ? 0 : v == 1 ? 1 : v == 3 ? 2 : 3)], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 512 + 4; k += kThreads) {
    const unsigned int x = sh[k];
    if (x) atomicAdd(k < 512 ? &hist[k] : &res[k - 512], (unsigned long long)x);
  }
}

}  // namespace

void launch_eval_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, BamPacking pk, uint64_t hash_mask, const int32_t *ref_map,
                      int64_t first, uint64_t *ptr, uint64_t *hash, int64_t *end, int32_t *gref, uint32_t *idx, hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_eval_keys, dim3(blocks_of(n_rec)), dim3(kThreads), 0, s, stream, rec, n_rec, pk.size_bits, hash_mask, ref_map, first, ptr,
                     hash, end, gref, idx);
}

void launch_eval_duplicates(const uint64_t *key, const uint32_t *perm, const uint64_t *t_ptr, int64_t n_truth, unsigned long long *dup,
                            hipStream_t s) {
  if (n_truth <= 1) return;
  hipLaunchKernelGGL(k_eval_duplicates, dim3(blocks_of(n_truth)), dim3(kThreads), 0, s, key, perm, t_ptr, n_truth, dup);
}

void launch_eval_join(const uint64_t *q_ptr, const uint64_t *q_hash, int64_t n_query, const uint64_t *key, const uint32_t *perm,
                      const uint64_t *t_ptr, int64_t n_truth, uint32_t *first, unsigned long long *cls, hipStream_t s) {
  if (n_query <= 0) return;
  hipLaunchKernelGGL(k_eval_join, dim3(blocks_of(n_query)), dim3(kThreads), 0, s, q_ptr, q_hash, n_query, key, perm, t_ptr, n_truth, first, cls);
}

void launch_eval_verdict(const uint64_t *t_ptr, const int64_t *t_end, const int32_t *t_gref, const uint32_t *first, int64_t n_truth,
                         const uint64_t *q_ptr, const int64_t *q_end, const int32_t *query_map, int32_t n_query_ref, int32_t permille,
                         uint8_t *verdict, unsigned long long *res, unsigned long long *hist, hipStream_t s) {
  if (n_truth <= 0) return;
  hipLaunchKernelGGL(k_eval_verdict, dim3(blocks_of(n_truth)), dim3(kThreads), 0, s, t_ptr, t_end, t_gref, first, n_truth, q_ptr, q_end, query_map,
                     n_query_ref, permille, verdict, res, hist);
}

}  // namespace pbsim
