// bam_aux.h -- the walk over a BAM record's aux fields (SAMv1 4.2.4) as device code does it, for the stages that read other
// people's records (through bam_cigar.h's resolve_cigar): by type, field after field, until what is wanted has been found or the fields
// end.  What is wanted: the array of the CG tag of type B,I (SAMv1 4.2.2), the value of the first NM tag of an integer type, or
// both.  A field that runs past the record or has an unknown type ends the walk with -1; fields behind the last wanted one are
// not looked at.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bam_fields.h"

namespace pbsim {

enum : int { kAuxCg = 1, kAuxNm = 2 };

struct BamAux {
  const uint8_t *cg;  // kAuxCg found: the tag's ops
  uint32_t n_cg;      //               and how many
  int64_t nm;         // kAuxNm found: the tag's value, sign-extended from its type (c C s S i I)
};

// The aux fields [a, end).  Returns the kAux* bits of what was found (0: nothing), or -1 where a field runs past the record or
// has an unknown type.
__device__ inline int bam_aux_walk(const uint8_t *a, const uint8_t *end, int want, BamAux *out) {
  int found = 0;
  while (a < end && (want & ~found)) {
    if (end - a < 3) return -1;
    const bool cg = (want & ~found & kAuxCg) && a[0] == 'C' && a[1] == 'G';
    const bool nm = (want & ~found & kAuxNm) && a[0] == 'N' && a[1] == 'M';
    const uint8_t t = a[2];
    a += 3;
    int64_t size;
    if (t == 'A' || t == 'c' || t == 'C') {
      size = 1;
    } else if (t == 's' || t == 'S') {
      size = 2;
    } else if (t == 'i' || t == 'I' || t == 'f') {
      size = 4;
    } else if (t == 'Z' || t == 'H') {
      const uint8_t *z = a;
      while (z < end && *z) z++;
      if (z >= end) return -1;
      size = z + 1 - a;
    } else if (t == 'B') {
      if (end - a < 5) return -1;
      const uint8_t sub = a[0];
      const int64_t count = ld32(a + 1);
      const int64_t each = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : sub == 'i' || sub == 'I' || sub == 'f' ? 4 : 0;
      if (each == 0) return -1;
      a += 5;
      size = count * each;
      if (size > end - a) return -1;
      if (cg && sub == 'I') {
        out->cg = a;
        out->n_cg = (uint32_t)count;
        found |= kAuxCg;
      }
    } else {
      return -1;
    }
    if (size > end - a) return -1;
    if (nm && (t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I')) {
      out->nm = t == 'c'   ? (int64_t)(int8_t)a[0]
                : t == 'C' ? (int64_t)a[0]
                : t == 's' ? (int64_t)(int16_t)ld16(a)
                : t == 'S' ? (int64_t)ld16(a)
                : t == 'i' ? (int64_t)(int32_t)ld32(a)
                           : (int64_t)ld32(a);
      found |= kAuxNm;
    }
    a += size;
  }
  return found;
}

}  // namespace pbsim
